// mpenv_manager.hpp — the reference's C++ Manager class (src/mgr.hpp:14-161)
// over the C ABI of mpenv.h, header-only, for C++ callers (headless/viewer
// style programs) that were written against madronaMPEnv::Manager.
//
// Same names, Config fields and method set; differences:
//   * madrona::py::Tensor -> madronaMPEnv::Tensor (ptr, type, dims, gpu id),
//     still a zero-copy view of engine-owned device memory (mgr.cpp:295-301).
//   * Errors throw std::runtime_error (the reference FATALs / asserts).
//   * Out of scope, declared with the reference's signatures
//     so callers written against mgr.hpp compile, and throwing
//     std::runtime_error when called: ExecMode::CPU (rejected at
//     construction), a non-null VizState* (the viewer), vizStep,
//     getWorldContext (Madrona's per-world ECS context, opaque Engine here),
//     setExploreAction and setCoarsePvPAction (Task::Explore and the
//     coarse-action path, neither on the Zone step graph).  Full-team
//     tensors, record/replay and event logs are implemented (fullTeam*Tensor
//     getters, Config log paths).  cpuJAXInit/Step are no-ops as in mgr.hpp.
//   * gpuStreamInit/Step take the HIP stream as void*.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "mpenv.h"

namespace madronaMPEnv {

enum class ExecMode : int32_t { CPU = MPENV_EXEC_CPU, CUDA = MPENV_EXEC_CUDA };

// types.hpp:45-51
enum class Task : uint32_t { Explore = 0, TDM = 1, Zone = 2, Turret = 3, ZoneCaptureDefend = 4 };

// sim_flags.hpp:7-20
enum class SimFlags : uint32_t {
    Default = 0,
    SpawnInMiddle = MPENV_SIMFLAG_SPAWN_IN_MIDDLE,
    RandomizeHPMagazine = MPENV_SIMFLAG_RANDOMIZE_HP_MAGAZINE,
    NavmeshSpawn = MPENV_SIMFLAG_NAVMESH_SPAWN,
    NoRespawn = MPENV_SIMFLAG_NO_RESPAWN,
    StaggerStarts = MPENV_SIMFLAG_STAGGER_STARTS,
    EnableCurriculum = MPENV_SIMFLAG_ENABLE_CURRICULUM,
    HardcodedSpawns = MPENV_SIMFLAG_HARDCODED_SPAWNS,
    RandomFlipTeams = MPENV_SIMFLAG_RANDOM_FLIP_TEAMS,
    StaticFlipTeams = MPENV_SIMFLAG_STATIC_FLIP_TEAMS,
    FullTeamPolicy = MPENV_SIMFLAG_FULL_TEAM_POLICY,
    SimEvalMode = MPENV_SIMFLAG_SIM_EVAL_MODE,
    SubZones = MPENV_SIMFLAG_SUB_ZONES,
};
inline SimFlags operator|(SimFlags a, SimFlags b) { return SimFlags((uint32_t)a | (uint32_t)b); }
inline SimFlags &operator|=(SimFlags &a, SimFlags b) { return a = a | b; }
inline SimFlags operator&(SimFlags a, SimFlags b) { return SimFlags((uint32_t)a & (uint32_t)b); }

struct Vector3 {
    float x, y, z;
    static Vector3 zero() { return { 0.f, 0.f, 0.f }; }
};

// Action components (types.hpp:173-183) and AgentPolicy.
struct PvPDiscreteAction { int32_t moveAmount, moveAngle, fire, stand; };
struct PvPAimAction { float yaw, pitch; };
struct PvPDiscreteAimAction { int32_t yaw, pitch; };
struct AgentPolicy { int32_t idx; };
struct ExploreAction { int32_t moveAmount, moveAngle, rotate, mantle; }; // types.hpp:166-171
struct CoarsePvPAction { int32_t moveAmount, moveAngle, facing; };       // types.hpp:205-209

// Opaque: the viewer's state (viz.hpp:16) and Madrona's per-world context
// (mgr.hpp:130); neither exists in this engine.
struct VizState;
struct Engine;

// mgr.hpp:16-24
struct MapConfig {
    const char *name;
    const char *collisionDataFile;
    const char *navmeshFile;
    const char *spawnDataFile;
    const char *zoneDataFile;
    Vector3 mapOffset;
    float mapRotation;
};

// madrona::py::Tensor equivalent: a view of engine-owned memory.
struct Tensor {
    enum class ElementType : int32_t { Int32 = MPENV_DTYPE_INT32, Float32 = MPENV_DTYPE_FLOAT32, UInt32 = MPENV_DTYPE_UINT32 };
    void *ptr = nullptr;
    ElementType type = ElementType::Float32;
    std::vector<int64_t> dims;
    int32_t gpuID = -1;
    void *devicePtr() const { return ptr; }
    int64_t numElements() const
    {
        int64_t n = 1;
        for (int64_t d : dims) n *= d;
        return n;
    }
    int64_t numBytes() const { return 4 * numElements(); }
};

// madrona::py::TrainInterface equivalent (mgr.cpp:2383-2431).
struct NamedTensor {
    std::string name;
    Tensor tensor;
};
struct TrainInterface {
    std::vector<NamedTensor> inputs;
    std::vector<NamedTensor> outputs;
};

class Manager {
public:
    // mgr.hpp:33-52
    struct Config {
        ExecMode execMode;
        int gpuID;
        uint32_t numWorlds;
        uint32_t randSeed;
        bool autoReset;
        SimFlags simFlags;
        Task taskType;
        uint32_t teamSize;
        uint32_t numPBTPolicies;
        uint32_t policyHistorySize;
        MapConfig map;
        bool highlevelMove = false;
        bool trainFlank = false;
        const char *replayLogPath = nullptr;
        const char *recordLogPath = nullptr;
        const char *eventLogPath = nullptr;
        const char *curriculumDataPath = nullptr;
        const char *policyWeightsPath = nullptr;
        uint32_t worldIDOffset = 0; // extension: first global world id (sharding)
        // extension: a map set (mpenv_maps.h): scene directory and number of worlds per range, the counts
        // summing to numWorlds; empty: `map`, as in mgr.hpp.  With maps, `map` is not read.
        std::vector<std::pair<std::string, uint32_t>> maps;
    };
    // one range of a map set, as the engine holds it (mapInfo)
    struct MapInfo {
        std::string scenePath;
        int32_t firstWorld, numWorlds;
        int32_t scene;     // index of the loaded scene; equal paths share one
        int32_t residency; // MPENV_SCENE_LDS or MPENV_SCENE_GLOBAL, in use
    };

    // mgr.hpp:54-56; viz must be null (there is no viewer)
    explicit Manager(const Config &cfg, VizState *viz = nullptr)
    {
        if (viz != nullptr) throw std::runtime_error("mpenv: the viewer (VizState) is not part of this engine");
        const std::string dir = cfg.maps.empty() ? sceneDir(cfg.map) : std::string();
        if (cfg.map.mapOffset.x != 0.f || cfg.map.mapOffset.y != 0.f || cfg.map.mapOffset.z != 0.f ||
            cfg.map.mapRotation != 0.f)
            throw std::runtime_error("mpenv: mapOffset/mapRotation must be zero (bindings.cpp:79-80)");
        if (cfg.highlevelMove) throw std::runtime_error("mpenv: highlevelMove is not implemented");
        mpenv_config c {};
        c.exec_mode = (int32_t)cfg.execMode;
        c.gpu_id = cfg.gpuID;
        c.num_worlds = cfg.numWorlds;
        c.rand_seed = cfg.randSeed;
        c.auto_reset = cfg.autoReset ? 1 : 0;
        c.sim_flags = (uint32_t)cfg.simFlags;
        c.task_type = (int32_t)cfg.taskType;
        c.team_size = cfg.teamSize;
        c.num_pbt_policies = cfg.numPBTPolicies;
        c.policy_history_size = cfg.policyHistorySize;
        c.scene_path = cfg.maps.empty() ? dir.c_str() : nullptr;
        c.train_flank = cfg.trainFlank ? 1 : 0;
        c.replay_log_path = cfg.replayLogPath;
        c.record_log_path = cfg.recordLogPath;
        c.event_log_path = cfg.eventLogPath;
        c.curriculum_data_path = cfg.curriculumDataPath;
        c.world_id_offset = cfg.worldIDOffset;
        if (cfg.maps.empty()) {
            check(mpenv_create(&c, &mgr_));
        } else {
            std::vector<mpenv_map_range> ranges;
            for (const auto &m : cfg.maps) ranges.push_back({ m.first.c_str(), m.second });
            check(mpenv_create_maps(&c, ranges.data(), (int32_t)ranges.size(), &mgr_));
        }
        execMode_ = cfg.execMode;
        // mgr.cpp loads policyWeightsPath into the sim's policyWeights; a
        // checkpoint that does not load is an error, as the reference's asserts
        if (cfg.policyWeightsPath != nullptr && mpenv_policy_load(mgr_, cfg.policyWeightsPath) != MPENV_OK) {
            const std::string why = mpenv_last_error();
            mpenv_destroy(mgr_);
            mgr_ = nullptr;
            throw std::runtime_error("mpenv: " + why);
        }
    }
    ~Manager() { mpenv_destroy(mgr_); }
    Manager(const Manager &) = delete;
    Manager &operator=(const Manager &) = delete;

    void init() { check(mpenv_init(mgr_)); }
    void step() { check(mpenv_step(mgr_)); }
    void vizStep() { outOfScope("vizStep (viewer)"); }
    inline void cpuJAXInit(void **, void **) {} // mgr.hpp:64-65: no-ops there too
    inline void cpuJAXStep(void **, void **) {}
    void gpuStreamInit(void *strm, void **buffers) { check(mpenv_gpu_stream_init(mgr_, strm, buffers)); }
    void gpuStreamStep(void *strm, void **buffers) { check(mpenv_gpu_stream_step(mgr_, strm, buffers)); }
    // extension: the Step graph enqueued on a caller stream without a sync
    void stepAsync(void *strm) { check(mpenv_step_async(mgr_, strm)); }

    // extension: in-sim policy inference (mpenv.h mpenv_policy_*): while a
    // checkpoint is loaded, step() first writes the actions of every agent
    // whose AgentPolicy.idx >= 0 (evalAgentPolicy, dnn.cpp:555-891)
    // League play (mpenv_policy_slots.h): one checkpoint per policy id in
    // [0, MPENV_POLICY_SLOTS); an id whose slot is empty, or past the last
    // slot, is served by id 0's checkpoint.  Loading into an occupied id
    // replaces that checkpoint alone.
    void loadPolicy(const char *dir, int policyId = 0) { check(mpenv_policy_load_slot(mgr_, policyId, dir)); }
    void unloadPolicy() { check(mpenv_policy_unload(mgr_)); } // every id
    void unloadPolicy(int policyId) { check(mpenv_policy_unload_slot(mgr_, policyId)); }
    bool policyLoaded() const
    {
        int32_t on = 0;
        check(mpenv_policy_loaded(mgr_, &on));
        return on != 0;
    }
    // the policy ids that hold a checkpoint, ascending
    std::vector<int> policySlots() const
    {
        uint32_t mask = 0;
        check(mpenv_policy_slots(mgr_, &mask));
        std::vector<int> ids;
        for (int s = 0; s < MPENV_POLICY_SLOTS; s++)
            if ((mask >> s) & 1u) ids.push_back(s);
        return ids;
    }
    // logits [A][37] f32 and actions [A][6] i32 (or null) are device pointers;
    // MPENV_POLICY_F32 (bit-equal to the reference, the default) or MPENV_POLICY_BF16 (the trunk and the
    // heads on the bf16 matrix cores: for frozen opponents); any time, loaded or not, nothing is reloaded
    void setPolicyPrecision(int precision) { check(mpenv_policy_set_precision(mgr_, precision)); }
    int policyPrecision() const
    {
        int32_t p = 0;
        check(mpenv_policy_precision(mgr_, &p));
        return p;
    }
    // extension: scene residency (mpenv_scene_residency.h).  MPENV_SCENE_AUTO, MPENV_SCENE_LDS (throws on a
    // scene that does not fit) or MPENV_SCENE_GLOBAL; between steps, the step graph is re-captured by the next
    void setSceneResidency(int mode) { check(mpenv_set_scene_residency(mgr_, mode)); }
    // the path in use: MPENV_SCENE_LDS or MPENV_SCENE_GLOBAL
    int sceneResidency() const
    {
        int32_t mode = 0;
        check(mpenv_scene_residency(mgr_, &mode));
        return mode;
    }
    // extension: map sets (mpenv_maps.h): the number of ranges (1 for a single-map manager) and one of them
    int numMaps() const
    {
        int32_t n = 0;
        check(mpenv_num_maps(mgr_, &n));
        return n;
    }
    MapInfo mapInfo(int range) const
    {
        mpenv_map_desc d;
        const char *path = nullptr;
        check(mpenv_map_info(mgr_, range, &d, &path));
        return { path ? path : "", d.first_world, d.num_worlds, d.scene, d.residency };
    }
    // extension: the egocentric depth camera (mpenv_camera.h): per agent a [height][width] depth (f32) and
    // label (u8) image behind every step and init while enabled; width and height multiples of 8 in [8, 128],
    // hfovDeg in (0, 170).  enableCamera again with another size replaces the camera.
    void enableCamera(int width, int height, float hfovDeg = 90.f)
    {
        const mpenv_camera_config c { width, height, hfovDeg, 0 };
        check(mpenv_camera_enable(mgr_, &c));
    }
    void disableCamera() { check(mpenv_camera_disable(mgr_)); }
    // whether a camera is enabled, and (cfg non-null) its configuration
    bool cameraEnabled(mpenv_camera_config *cfg = nullptr) const
    {
        int32_t on = 0;
        check(mpenv_camera_enabled(mgr_, cfg, &on));
        return on != 0;
    }
    // the images of the current state, without a step; strm null: the manager's own stream, waited for
    void renderCamera(void *strm = nullptr) { check(mpenv_camera_render(mgr_, strm)); }
    // device pointers to [A][height][width] f32 / u8 and the three dims (may be null); they hold until the
    // next enableCamera or disableCamera
    float *cameraDepth(int64_t *dims = nullptr) const
    {
        return static_cast<float *>(cameraImage(MPENV_CAMERA_DEPTH, dims));
    }
    uint8_t *cameraLabel(int64_t *dims = nullptr) const
    {
        return static_cast<uint8_t *>(cameraImage(MPENV_CAMERA_LABEL, dims));
    }
    // extension: the league scheduler (mpenv_league.h): standings int64 [P+1][P+1][8] and, by draw mode,
    // a weighted redraw of the policy ids of every world that ends an episode, behind every step and init.
    // Needs auto_reset; enableLeague again replaces the league.
    void enableLeague(int numPolicies, int32_t draw = MPENV_LEAGUE_DRAW_TEAM1, uint32_t seed = 0)
    {
        const mpenv_league_config c { numPolicies, draw, seed, 0 };
        check(mpenv_league_enable(mgr_, &c));
    }
    void disableLeague() { check(mpenv_league_disable(mgr_)); }
    // whether a league is enabled, and (cfg non-null) its configuration
    bool leagueConfig(mpenv_league_config *cfg = nullptr) const
    {
        int32_t on = 0;
        check(mpenv_league_enabled(mgr_, cfg, &on));
        return on != 0;
    }
    // device pointers and dims (may be null); they hold until the next enableLeague or disableLeague
    int64_t *leagueTable(int64_t *dims = nullptr) const
    {
        return static_cast<int64_t *>(leagueTensor(MPENV_LEAGUE_TABLE, dims));
    }
    int32_t *leagueWeights(int64_t *dims = nullptr) const
    {
        return static_cast<int32_t *>(leagueTensor(MPENV_LEAGUE_WEIGHTS, dims));
    }
    uint32_t *leagueDraws(int64_t *dims = nullptr) const
    {
        return static_cast<uint32_t *>(leagueTensor(MPENV_LEAGUE_DRAWS, dims));
    }
    // zeroes the table; asynchronous on strm (null: the manager's own stream)
    void clearLeague(void *strm = nullptr) { check(mpenv_league_clear(mgr_, strm)); }
    // extension: the live curriculum pool (mpenv_curriculum.h): [ranges][capacity] snapshots in device
    // memory that episode starts read in place, refreshed behind every step from the running batch.
    // After init(); enableCurriculumPool again replaces the pool.
    void enableCurriculumPool(int capacity, int period = 64, int stepLo = 0, int stepHi = 2999 /* episodeLen - 1 */,
                              uint32_t need = 0, uint32_t seed = 0)
    {
        const mpenv_curriculum_pool_config c { capacity, period, stepLo, stepHi, need, seed };
        check(mpenv_curriculum_pool_enable(mgr_, &c));
    }
    void disableCurriculumPool() { check(mpenv_curriculum_pool_disable(mgr_)); }
    // period, window, need and seed; cfg.capacity must be the enabled one
    void configureCurriculumPool(const mpenv_curriculum_pool_config &cfg)
    {
        check(mpenv_curriculum_pool_configure(mgr_, &cfg));
    }
    // whether a pool is enabled, and (cfg non-null) its configuration
    bool curriculumPoolConfig(mpenv_curriculum_pool_config *cfg = nullptr) const
    {
        int32_t on = 0;
        check(mpenv_curriculum_pool_enabled(mgr_, cfg, &on));
        return on != 0;
    }
    // device pointers and dims (may be null); they hold until the next enable or disable
    mpenv_curriculum_snapshot *curriculumPool(int64_t *dims = nullptr) const
    {
        return static_cast<mpenv_curriculum_snapshot *>(curriculumPoolTensor(MPENV_CURRICULUM_POOL, dims));
    }
    uint32_t *curriculumPoolTicks(int64_t *dims = nullptr) const
    {
        return static_cast<uint32_t *>(curriculumPoolTensor(MPENV_CURRICULUM_TICKS, dims));
    }
    uint32_t curriculumPoolTick() const
    {
        uint32_t t = 0;
        check(mpenv_curriculum_pool_tick(mgr_, &t));
        return t;
    }
    void setCurriculumPool(const mpenv_curriculum_snapshot *host, int n, int mapRange = 0, int firstSlot = 0)
    {
        check(mpenv_curriculum_pool_set(mgr_, mapRange, firstSlot, n, host));
    }
    // every agent through policyId's checkpoint
    void policyForward(float *logits, int32_t *actions = nullptr, void *strm = nullptr, int policyId = 0)
    {
        check(mpenv_policy_forward_slot(mgr_, policyId, logits, actions, strm));
    }

    // extension: world checkpoints (mpenv.h mpenv_state_*).  snapshot / worldMap
    // are device pointers; worldMap null restores every world, strm null is
    // the manager's own stream.  loadState never synchronises: a refused
    // snapshot or map shows in stateError() (MPENV_STATE_ERR_* bits).
    int64_t stateBytes() const
    {
        int64_t b = 0;
        check(mpenv_state_bytes(mgr_, &b));
        return b;
    }
    void saveState(void *snapshot, void *strm = nullptr) { check(mpenv_state_save(mgr_, snapshot, strm)); }
    void loadState(const void *snapshot, const int32_t *worldMap = nullptr, void *strm = nullptr)
    {
        check(mpenv_state_load(mgr_, snapshot, worldMap, strm));
    }
    uint32_t stateError()
    {
        uint32_t e = 0;
        check(mpenv_state_error(mgr_, &e));
        return e;
    }

    Tensor resetTensor() const { return get(MPENV_EXPORT_RESET); }
    Tensor simControlTensor() const { return get(MPENV_EXPORT_SIM_CONTROL); }
    Tensor matchResultTensor() const { return get(MPENV_EXPORT_MATCH_RESULT); }
    Tensor pvpDiscreteActionTensor() const { return get(MPENV_EXPORT_PVP_DISCRETE_ACTION); }
    Tensor pvpAimActionTensor() const { return get(MPENV_EXPORT_PVP_AIM_ACTION); }
    Tensor pvpDiscreteAimActionTensor() const { return get(MPENV_EXPORT_PVP_DISCRETE_AIM_ACTION); }
    Tensor exploreActionTensor() const { return get(MPENV_EXPORT_EXPLORE_ACTION); }
    Tensor rewardTensor() const { return get(MPENV_EXPORT_REWARD); }
    Tensor doneTensor() const { return get(MPENV_EXPORT_DONE); }
    Tensor policyAssignmentTensor() const { return get(MPENV_EXPORT_AGENT_POLICY); }
    Tensor worldCurriculumTensor() const { return get(MPENV_EXPORT_WORLD_CURRICULUM); }
    Tensor selfObservationTensor() const { return get(MPENV_EXPORT_SELF_OBSERVATION); }
    Tensor filtersStateObservationTensor() const { return get(MPENV_EXPORT_FILTERS_STATE); }
    Tensor teammateObservationsTensor() const { return get(MPENV_EXPORT_TEAMMATE_OBSERVATIONS); }
    Tensor opponentObservationsTensor() const { return get(MPENV_EXPORT_OPPONENT_OBSERVATIONS); }
    Tensor opponentLastKnownObservationsTensor() const { return get(MPENV_EXPORT_OPPONENT_LAST_KNOWN_OBSERVATIONS); }
    Tensor selfPositionTensor() const { return get(MPENV_EXPORT_SELF_POSITION); }
    Tensor teammatePositionObservationsTensor() const { return get(MPENV_EXPORT_TEAMMATE_POSITIONS); }
    Tensor opponentPositionObservationsTensor() const { return get(MPENV_EXPORT_OPPONENT_POSITIONS); }
    Tensor opponentLastKnownPositionObservationsTensor() const
    {
        return get(MPENV_EXPORT_OPPONENT_LAST_KNOWN_POSITIONS);
    }
    Tensor opponentMasksTensor() const { return get(MPENV_EXPORT_OPPONENT_MASKS); }
    Tensor fwdLidarTensor() const { return get(MPENV_EXPORT_FWD_LIDAR); }
    Tensor rearLidarTensor() const { return get(MPENV_EXPORT_REAR_LIDAR); }
    Tensor agentMapTensor() const { return get(MPENV_EXPORT_AGENT_MAP); }
    Tensor unmaskedAgentMapTensor() const { return get(MPENV_EXPORT_UNMASKED_AGENT_MAP); }
    Tensor hpTensor() const { return get(MPENV_EXPORT_HP); }
    Tensor magazineTensor() const { return get(MPENV_EXPORT_MAGAZINE); }
    Tensor aliveTensor() const { return get(MPENV_EXPORT_ALIVE); }
    Tensor rewardHyperParamsTensor() const { return get(MPENV_EXPORT_REWARD_HYPER_PARAMS); }
    // FullTeamInterface (mgr.hpp:110-120)
    Tensor fullTeamActionTensor() const { return get(MPENV_EXPORT_FULL_TEAM_ACTIONS); }
    Tensor fullTeamGlobalObservationsTensor() const { return get(MPENV_EXPORT_FULL_TEAM_GLOBAL); }
    Tensor fullTeamPlayerObservationsTensor() const { return get(MPENV_EXPORT_FULL_TEAM_PLAYERS); }
    Tensor fullTeamEnemyObservationsTensor() const { return get(MPENV_EXPORT_FULL_TEAM_ENEMIES); }
    Tensor fullTeamLastKnownEnemyObservationsTensor() const
    {
        return get(MPENV_EXPORT_FULL_TEAM_LAST_KNOWN_ENEMIES);
    }
    Tensor fullTeamFwdLidarTensor() const { return get(MPENV_EXPORT_FULL_TEAM_FWD_LIDAR); }
    Tensor fullTeamRearLidarTensor() const { return get(MPENV_EXPORT_FULL_TEAM_REAR_LIDAR); }
    Tensor fullTeamRewardTensor() const { return get(MPENV_EXPORT_FULL_TEAM_REWARD); }
    Tensor fullTeamDoneTensor() const { return get(MPENV_EXPORT_FULL_TEAM_DONE); }
    Tensor fullTeamPolicyAssignmentTensor() const { return get(MPENV_EXPORT_FULL_TEAM_POLICY_ASSIGNMENTS); }

    TrainInterface trainInterface() const
    {
        TrainInterface ti;
        int32_t ni = 0, no = 0;
        check(mpenv_train_interface_size(&ni, &no));
        for (int io = 0; io < 2; io++) {
            for (int32_t k = 0; k < (io ? no : ni); k++) {
                const char *name = nullptr;
                int32_t id = 0;
                check(mpenv_train_interface_entry(io, k, &name, &id));
                (io ? ti.outputs : ti.inputs).push_back({ name, get(id) });
            }
        }
        return ti;
    }

    ExecMode execMode() const { return execMode_; }

    Engine &getWorldContext(int32_t) { outOfScope("getWorldContext (Madrona ECS context)"); }

    void triggerReset(int32_t world_idx) { check(mpenv_trigger_reset(mgr_, world_idx)); }
    void setExploreAction(int32_t, ExploreAction) { outOfScope("setExploreAction (Task::Explore)"); }
    void setCoarsePvPAction(int32_t, int32_t, CoarsePvPAction) { outOfScope("setCoarsePvPAction"); }
    void setPvPAction(int32_t world_idx, int32_t agent_idx, PvPDiscreteAction discrete, PvPAimAction aim,
                      PvPDiscreteAimAction aim_discrete)
    {
        const int32_t d[4] = { discrete.moveAmount, discrete.moveAngle, discrete.fire, discrete.stand };
        const float a[2] = { aim.yaw, aim.pitch };
        const int32_t ad[2] = { aim_discrete.yaw, aim_discrete.pitch };
        check(mpenv_set_pvp_action(mgr_, world_idx, agent_idx, d, a, ad));
    }
    void setHP(int32_t world_idx, int32_t agent_idx, int32_t hp) { check(mpenv_set_hp(mgr_, world_idx, agent_idx, hp)); }
    bool isReplayFinished()
    {
        int32_t f = 0;
        check(mpenv_is_replay_finished(mgr_, &f));
        return f != 0;
    }
    void setAgentPolicy(int32_t world_idx, int32_t agent_idx, AgentPolicy policy)
    {
        check(mpenv_set_agent_policy(mgr_, world_idx, agent_idx, policy.idx));
    }
    void setUniformAgentPolicy(AgentPolicy policy) { check(mpenv_set_uniform_agent_policy(mgr_, policy.idx)); }

    mpenv_manager *handle() const { return mgr_; }

private:
    [[noreturn]] static void outOfScope(const char *what)
    {
        throw std::runtime_error(std::string("mpenv: ") + what + " is out of scope for this engine (DESIGN.md §8)");
    }

    static void check(int rc)
    {
        if (rc != MPENV_OK) throw std::runtime_error(std::string("mpenv: ") + mpenv_last_error());
    }

    void *cameraImage(int32_t which, int64_t *dims) const
    {
        void *p = nullptr;
        int32_t dtype = 0, ndim = 0;
        int64_t d[8] = {};
        check(mpenv_camera_tensor(mgr_, which, &p, &dtype, &ndim, d, nullptr));
        for (int k = 0; dims && k < ndim; k++) dims[k] = d[k];
        return p;
    }

    void *leagueTensor(int32_t which, int64_t *dims) const
    {
        void *p = nullptr;
        int32_t dtype = 0, ndim = 0;
        int64_t d[8] = {};
        check(mpenv_league_tensor(mgr_, which, &p, &dtype, &ndim, d, nullptr));
        for (int k = 0; dims && k < ndim; k++) dims[k] = d[k];
        return p;
    }

    void *curriculumPoolTensor(int32_t which, int64_t *dims) const
    {
        void *p = nullptr;
        int32_t dtype = 0, ndim = 0;
        int64_t d[8] = {};
        check(mpenv_curriculum_pool_tensor(mgr_, which, &p, &dtype, &ndim, d, nullptr));
        for (int k = 0; dims && k < ndim; k++) dims[k] = d[k];
        return p;
    }

    // bindings.cpp:56-78 builds the four paths from one scene directory;
    // accept exactly that layout.
    static std::string sceneDir(const MapConfig &m)
    {
        if (!m.collisionDataFile) throw std::runtime_error("mpenv: MapConfig.collisionDataFile is required");
        std::string c = m.collisionDataFile;
        const std::string suffix = "/collisions.bin";
        if (c.size() < suffix.size() || c.compare(c.size() - suffix.size(), suffix.size(), suffix) != 0)
            throw std::runtime_error("mpenv: collisionDataFile must be <scene>/collisions.bin");
        std::string dir = c.substr(0, c.size() - suffix.size());
        auto same = [&](const char *p, const char *name) {
            return p == nullptr || std::string(p) == dir + "/" + name;
        };
        if (!same(m.navmeshFile, "navmesh.bin") || !same(m.spawnDataFile, "spawns.bin") ||
            !same(m.zoneDataFile, "zones.bin"))
            throw std::runtime_error("mpenv: scene files must share one directory (bindings.cpp:56-78 layout)");
        return dir;
    }

    Tensor get(int32_t id) const
    {
        Tensor t;
        int32_t dt = 0, nd = 0, gpu = -1;
        int64_t dims[8];
        check(mpenv_export_tensor(mgr_, id, &t.ptr, &dt, &nd, dims, &gpu));
        t.type = Tensor::ElementType(dt);
        t.dims.assign(dims, dims + nd);
        t.gpuID = gpu;
        return t;
    }

    mpenv_manager *mgr_ = nullptr;
    ExecMode execMode_ = ExecMode::CUDA;
};

} // namespace madronaMPEnv
