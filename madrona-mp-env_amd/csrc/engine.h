// engine.h — device state layout of the MI355X engine.
//
// The reference stores per-entity components in Madrona ECS archetype
// columns (PvPAgent, types.hpp:932-995) and per-world singletons
// (sim.hpp:81-191).  Here every per-agent internal field is its own
// structure-of-arrays column indexed by the global agent id
// g = world * N + agent (N = 2 * teamSize, team 0 offsets first,
// level_gen.cpp:148-162), so lanes that own consecutive agents issue
// coalesced loads.  Exported components keep the reference's
// array-of-struct column layout (tensor dims of mgr.cpp:1965-2381) because
// they are the drop-in boundary.
#pragma once

#include <cstdint>

#include "mpenv.h"
#include "mpenv_core.h"
#include "scene.h"

namespace mpenv {

constexpr int kMaxTeamSize = 6;
constexpr int kMaxAgents = 2 * kMaxTeamSize;
constexpr int kMaxZones = 5;
constexpr int kGridW = 81;
constexpr int kGridCells = kGridW * kGridW;
// ExploreTracker as a per-agent bitset over the 81 x 81 cells: bit = the
// cell holds the agent's current episode index (exploreEp).  Exact for
// exploreVisitedSystem (sim.cpp:3508-3536), see DESIGN.md §2.  Cells are
// grouped in 8 x 8 tiles, one u64 each (11 x 11 tiles, 968 B per agent);
// the tile the agent stands in lives in SoA columns (exploreTile,
// exploreLo / exploreHi), so consecutive steps inside one tile (240 x 240
// units) touch only coalesced columns and the row is read / written once
// per tile change.
constexpr int kExploreTilesX = 11;
constexpr int kExploreTiles = kExploreTilesX * kExploreTilesX;
constexpr int kSelfObs = 43;
constexpr int kOtherObs = 32;
constexpr int kFwdRays = 64;   // 2 x 32
constexpr int kRearRays = 16;  // 2 x 8
constexpr int kLidarRays = kFwdRays + kRearRays;
constexpr int kMaxCrumbs = 128;
constexpr int kMinSpawnTrack = 128; // SpawnUsageCounter::maxNumSpawns (types.hpp:96)
constexpr int kMaxBVHStack = 16; // register byte-stack capacity (LDS-resident scenes)
constexpr int kMaxGlobalStack = 64; // WideStack capacity (global-resident scenes); the oracle's stack holds as many
constexpr int kMaxLdsNodes = 256;   // a byte-stack entry holds a node index
// k_vis's occluder hints are uint16_t triangle indices, 0xffff = none
constexpr int kMaxSceneTris = 0xfffe;
constexpr size_t kLdsBudget = 64 * 1024; // dynamic LDS a block may ask for without a function attribute

#define MP_AGENT_F32(X) \
    X(px) X(py) X(pz) X(vx) X(vy) X(vz) X(rw) X(rx) X(ry) X(rz) \
    X(ayaw) X(apitch) X(aw) X(ax) X(ay) X(az) X(maxVel) X(minDistZone) \
    X(firedT) X(bcPenalty) X(sx) X(sy) X(sz) X(dyv) X(dpv) X(minDistSub)

#define MP_AGENT_I32(X) \
    X(curPose) X(tgtPose) X(transRem) X(rngA) X(rngB) X(rngCtr) X(landedOn) \
    X(respawnSteps) X(autohealSteps) X(flags) X(wasShot) X(weapon) X(bcLast) \
    X(bcSteps) X(newCells) X(exploreEp) X(exploreTile) X(exploreLo) X(exploreHi)

#define MP_WORLD_I32(X) \
    X(teamA) X(curStep) X(finished) X(curZone) X(controlling) X(contested) \
    X(captured) X(earned) X(zoneSteps) X(stepsUntilPoint) X(episode) \
    X(episodeCounter) X(wRngA) X(wRngB) X(wRngCtr) X(filtAct0) X(filtAct1) \
    X(filtMatched0) X(filtMatched1) X(episodeCurr) X(numCrumbs) X(nextCrumbId) \
    X(crumbOverflow) X(curTier) X(curSpawnIdx) X(spawnCurriculum) \
    X(matchValid) X(evLogged) X(evMask) X(snapWritten) X(subState)

#define MP_WORLD_F32(X) \
    X(teamRew0) X(teamRew1) X(goalMin0) X(goalMin1) X(goalTeam0) X(goalTeam1)

// The buffer table: every other device buffer of DevState, declared once
// (dmg, resetKeys and the optional logs apart, see DevState).
//   X(member, element type, row kind, row shape...)
//   E(member, element type, row kind, MPENV_EXPORT_* id, row shape...)   exported
// A row holds the product of its shape in elements.  An exported buffer's
// tensor dims are its row count followed by that shape, so a trailing 1 is
// part of it where the reference's dims have one (mgr.cpp:1965-2381).
// DevState's members, the row:: constants below, and in manager.cpp
// allocState, sliceState and the export layout / pointers are expansions of
// these lists: a new buffer is one line here.  A shape may name T (the team
// size) and trackLen (SceneDev::spawnTrackLen), which the run-time
// expansions define; exported shapes are compile-time constants.  The lists
// are in member and allocation order, cut in three where allocState
// allocates by hand in between.
enum RowKind {
    kPerAgent,  // A rows; a world range starts at row w0 * N
    kPerWorld,  // W rows; at row w0
    kPerTeam,   // 2 W rows, one per (world, team); at row 2 * w0
    kUnsliced,  // one row shared by every world range
};

constexpr int64_t bufRows(RowKind k, int64_t W, int64_t N)
{
    return k == kPerAgent ? W * N : k == kPerWorld ? W : k == kPerTeam ? 2 * W : 1;
}

// first row of the world range that starts at world w0
constexpr int64_t bufFirstRow(RowKind k, int64_t w0, int64_t N)
{
    return k == kUnsliced ? 0 : bufRows(k, w0, N);
}

template <typename... D>
constexpr int64_t rowElems(D... d)
{
    return (int64_t(1) * ... * int64_t(d));
}

#define MP_BUFS_A(X, E) \
    X(visMask, uint8_t, kPerAgent, 1) /* OpponentsVisibility, bit k = sees opponent k */

// visOcc: k_vis occluder hint per (agent, opponent slot, sample point): the
// triangle that last ended that line-of-sight ray (0xffff: none).  A
// performance hint only -- any value gives the same answer (geom_dev.h
// visibleRayD) -- so it is never reset.
// exploreBits: ExploreTracker tiles for episode exploreEp (the tile
// exploreTile is current in exploreLo / exploreHi).
#define MP_BUFS_B(X, E) \
    X(visOcc, uint16_t, kPerAgent, T, 4) \
    X(exploreBits, uint64_t, kPerAgent, kExploreTiles) \
    X(filtLast, int32_t, kPerWorld, 2, 3) /* FiltersMatchState::lastMatches (3 filters used) */ \
    X(zoneStats, int32_t, kPerWorld, 5, 5)

#define MP_BUFS_C(X, E) \
    X(spawnTrack, uint32_t, kPerWorld, 3, trackLen) /* SpawnUsageCounter */ \
    X(crumbs, float4, kPerWorld, kMaxCrumbs, 2) /* {x,y,z,penalty},{team,offset,id,-} */ \
    /* Exported columns (reference layouts) */ \
    E(reset, int32_t, kPerWorld, MPENV_EXPORT_RESET, 1) \
    E(worldCurr, int32_t, kPerWorld, MPENV_EXPORT_WORLD_CURRICULUM, 1) \
    E(matchResult, int32_t, kPerWorld, MPENV_EXPORT_MATCH_RESULT, 30) \
    E(exploreAction, int32_t, kPerAgent, MPENV_EXPORT_EXPLORE_ACTION, 4) \
    E(discreteAction, int32_t, kPerAgent, MPENV_EXPORT_PVP_DISCRETE_ACTION, 4) \
    E(aimAction, float, kPerAgent, MPENV_EXPORT_PVP_AIM_ACTION, 1, 2) \
    E(discreteAim, int32_t, kPerAgent, MPENV_EXPORT_PVP_DISCRETE_AIM_ACTION, 2) \
    E(policy, int32_t, kPerAgent, MPENV_EXPORT_AGENT_POLICY, 1) \
    X(botAction, int32_t, kPerAgent, 7) \
    E(reward, float, kPerAgent, MPENV_EXPORT_REWARD, 1) \
    E(done, int32_t, kPerAgent, MPENV_EXPORT_DONE, 1) \
    E(selfObs, float, kPerAgent, MPENV_EXPORT_SELF_OBSERVATION, kSelfObs) \
    E(filters, float, kPerAgent, MPENV_EXPORT_FILTERS_STATE, 1) \
    E(tmObs, float, kPerAgent, MPENV_EXPORT_TEAMMATE_OBSERVATIONS, 5, kOtherObs) \
    E(oppObs, float, kPerAgent, MPENV_EXPORT_OPPONENT_OBSERVATIONS, 6, kOtherObs) \
    E(lkObs, float, kPerAgent, MPENV_EXPORT_OPPONENT_LAST_KNOWN_OBSERVATIONS, 6, kOtherObs) \
    E(selfPos, float, kPerAgent, MPENV_EXPORT_SELF_POSITION, 3) \
    E(tmPos, float, kPerAgent, MPENV_EXPORT_TEAMMATE_POSITIONS, 5, 3) \
    E(oppPos, float, kPerAgent, MPENV_EXPORT_OPPONENT_POSITIONS, 6, 3) \
    E(lkPos, float, kPerAgent, MPENV_EXPORT_OPPONENT_LAST_KNOWN_POSITIONS, 6, 3) \
    E(masks, float, kPerAgent, MPENV_EXPORT_OPPONENT_MASKS, 6, 1) \
    E(fwdLidar, float, kPerAgent, MPENV_EXPORT_FWD_LIDAR, 2, 32, 4) \
    E(rearLidar, float, kPerAgent, MPENV_EXPORT_REAR_LIDAR, 2, 8, 4) \
    /* never written, as in the reference; also MPENV_EXPORT_UNMASKED_AGENT_MAP */ \
    E(agentMap, float, kPerAgent, MPENV_EXPORT_AGENT_MAP, 16, 16, 4) \
    E(hp, float, kPerAgent, MPENV_EXPORT_HP, 1) \
    E(alive, float, kPerAgent, MPENV_EXPORT_ALIVE, 1) \
    E(magazine, int32_t, kPerAgent, MPENV_EXPORT_MAGAZINE, 2) \
    E(rewardCoefs, float, kPerAgent, MPENV_EXPORT_REWARD_HYPER_PARAMS, 9) \
    X(trainCtrl, int32_t, kUnsliced, 3) /* MPENV_EXPORT_SIM_CONTROL, dims { 3 } */ \
    /* FullTeamInterface columns, one row per (world, team) (types.hpp:1040-1152); */ \
    /* ftActions and ftPolicy are inputs the step never reads */ \
    E(ftActions, int32_t, kPerTeam, MPENV_EXPORT_FULL_TEAM_ACTIONS, 6, 4) \
    E(ftGlobal, float, kPerTeam, MPENV_EXPORT_FULL_TEAM_GLOBAL, MPENV_FT_GLOBAL_DIM) \
    E(ftPlayers, float, kPerTeam, MPENV_EXPORT_FULL_TEAM_PLAYERS, 6, MPENV_FT_PLAYER_DIM) \
    E(ftEnemies, float, kPerTeam, MPENV_EXPORT_FULL_TEAM_ENEMIES, 6, MPENV_FT_ENEMY_DIM) \
    E(ftLastKnown, float, kPerTeam, MPENV_EXPORT_FULL_TEAM_LAST_KNOWN_ENEMIES, 6, MPENV_FT_COMMON_DIM) \
    E(ftFwdLidar, float, kPerTeam, MPENV_EXPORT_FULL_TEAM_FWD_LIDAR, 6, 2, 32, 4) \
    E(ftRearLidar, float, kPerTeam, MPENV_EXPORT_FULL_TEAM_REAR_LIDAR, 6, 2, 8, 4) \
    E(ftReward, float, kPerTeam, MPENV_EXPORT_FULL_TEAM_REWARD, 1) \
    E(ftDone, int32_t, kPerTeam, MPENV_EXPORT_FULL_TEAM_DONE, 1) \
    E(ftPolicy, int32_t, kPerTeam, MPENV_EXPORT_FULL_TEAM_POLICY_ASSIGNMENTS, 1)

#define MP_BUFS(X, E) MP_BUFS_A(X, E) MP_BUFS_B(X, E) MP_BUFS_C(X, E)
#define MP_BUF_SKIP(...)

// Elements per row of each exported buffer (row::lkPos == 18, ...)
namespace row {
#define MP_ROW(n, type, kind, id, ...) constexpr int n = (int)rowElems(__VA_ARGS__);
MP_BUFS(MP_BUF_SKIP, MP_ROW)
#undef MP_ROW
} // namespace row
static_assert(row::fwdLidar == kFwdRays * 4 && row::rearLidar == kRearRays * 4, "lidar rows are float4 per ray");

// Agent flag bits (CombatState booleans, types.hpp:510-528)
enum : int32_t {
    kFlagSuccessfulKill = 1,
    kFlagWasKilled = 2,
    kFlagInZone = 4,
    kFlagHasDied = 8,
    kFlagReloadedFullMag = 16,
    kFlagInSubZone = 32,
};

struct DevState {
    int32_t W, N, T;
    uint32_t nMagic;       // ceil(2^32 / N): g / N = umulhi(g, nMagic) for g < 2^32 / N^2
    int64_t A;
    int64_t dmgStride;     // row stride of dmg (all agents of the manager)

#define MP_DECL_F(n) float *n;
#define MP_DECL_I(n) int32_t *n;
    MP_AGENT_F32(MP_DECL_F)
    MP_AGENT_I32(MP_DECL_I)
    MP_WORLD_I32(MP_DECL_I)
    MP_WORLD_F32(MP_DECL_F)
#undef MP_DECL_F
#undef MP_DECL_I

    float *dmg;            // [6][A] DamageDealt, row stride dmgStride
#define MP_DECL(n, type, ...) type *n;
    MP_BUFS(MP_DECL, MP_DECL)
#undef MP_DECL

    // Record / replay / event logs (allocated only when enabled)
    mpenv_step_log *recordLog;             // [W] written by the step
    const mpenv_step_log *replayLog;       // [W] read by the step
    mpenv_game_event *events;              // [W][evStride] slots: 2 per agent + capture
    mpenv_packed_step_snapshot *snapshots; // [W]
    int32_t evStride;                      // 2 * N + 1

    // Per agent: combat RNG key + first draw keys of a coming reset (k_sim)
    mp::RandKey *resetKeys; // [A][11]

    // Workload counters (mpenv_enable_stats), null when off: see StatId.
    unsigned long long *stats;
    // k_obs does nothing while (*obsGate & MPENV_WIRE_ERR_DESYNC): a learner
    // shadow whose wire history broke (wire.hip wireOk); null on the step path.
    const uint32_t *obsGate;
    // gpuStreamStep's caller buffers (OutTab): while outTab->on, k_obs writes
    // its pure outputs there instead of into the engine's exports, and
    // k_lidar writes the lidar rows there too; outBase = this state's first
    // agent in those buffers (world groups).  Null on a wire view.
    const struct OutTab *outTab;
    int64_t outBase;
};

// The caller's trainInterface output buffers k_obs / k_lidar write directly
// during a gpuStreamStep (mgr.cpp:614-645 copies them from the engine's
// exports instead).  A device table, so the captured step graph's kernel
// arguments never change: gpuStreamStep sets it (on = 1, the call's
// pointers) in front of the step and clears it behind it, both from inside
// its input / output copy launches (CopyBatch::tabDst).
struct OutTab {
    int32_t on, pad;
    float *masks, *filters, *selfObs, *selfPos, *tmObs, *tmPos, *oppObs, *oppPos, *fwdLidar, *rearLidar;
    // the two agent-map outputs (constant zeros, as the reference copies
    // them): zero-filled by k_lidar's forward waves, 8 KB per agent of
    // stores that need no loads, issued beside its VALU-bound traversals
    float *agentMap0, *agentMap1;
};

// Per-step workload counters accumulated by the kernels in stats mode
// (bench.py's workload window; never on in the timed region).
enum StatId {
    kStatAliveAgents = 0, // agents alive when k_move runs
    kStatLosPairs = 1,    // (viewer, opponent) pairs with both alive
    kStatLosRays = 2,     // visibility rays traced after the view/frustum tests
    kStatLosSeen = 3,     // of those, rays that found their target
    kStatSphereCasts = 4, // MeshBVH::sphereCast calls (k_move)
    kStatShots = 5,       // fireSystem rays (k_sim)
    kStatHits = 6,        // agents that took damage (applyDmgSystem)
    kStatKills = 7,       // agents killed (alive -> hp <= 0)
    kStatLkRows = 8,      // last-known rows k_obs wrote (knows / cleared on death)
    kStatLosTraced = 9,   // LOS rays that needed a BVH traversal (not decided by the target test or hint)
    kNumStats = 10,
};

struct ZOBBDev {
    mp::Vec3 pMin, pMax;
    float rotation;
};

struct GoalRegionDev {
    ZOBBDev sub[3];
    int32_t numSub;
    int32_t attackerTeam;
    float rewardStrength;
};

// Zone / sub-zone / goal tables in global memory.  Device code indexes them
// with per-world values (the current zone, a sub-zone id): indexing the
// by-value kernel-argument arrays of SceneDev dynamically makes the compiler
// copy the whole argument struct into registers (k_sim's zoneSystem alone
// needed ~200 VGPRs that way).
// A rotated box's frame: qinv(angleAxis(rot, up)) and its corners rotated
// into it -- what zoneSystem / distToZOBB recompute per call.  Filled on the
// device by k_scene_frames with the same functions, so every bit matches.
struct FrameDev {
    mp::Quat toFrame;
    mp::Vec3 pMin, pMax;
};

struct SceneTables {
    mp::AABB zoneAABB[kMaxZones];
    float zoneRot[kMaxZones];
    ZOBBDev subZones[8];
    GoalRegionDev goals[4];
    int32_t zoneGoalTri[kMaxZones];
    FrameDev zoneFrame[kMaxZones];
    FrameDev goalFrame[4][3];
};

// Read-only scene + task constants, passed by value as a kernel argument.
struct SceneDev {
    const SceneTables *tab; // device copy of the arrays below (set after scene upload)
    const BVHNode *nodes;
    const BVHNode *octNodes; // [8][numLidarNodes] octant node images of the lidar tree (scene.h octantNodeImages)
    const float *lidarVerts; // the lidar tree's triangles, 3 floats per vertex (scene.h Scene::lidarVerts)
    int32_t numLidarNodes, numLidarVerts;
    const float *verts;     // 3 floats per vertex, 3 vertices per triangle
    // Per triangle, ray-independent terms of sphereCastTriangle
    // (mesh_bvh.inl:885-1127): unit normal xyz, |normal|, |e01|^2, |e02|^2,
    // |e12|^2, 0 -- computed on the host with the same mpenv_core.h
    // expressions the traversal would evaluate (bit-identical).
    const float *triPre;
    int32_t numNodes;
    int32_t numVerts;
    mp::AABB worldBounds;
    float maxDist;
    float frustum[4];
    const Spawn *aSpawns;
    const Spawn *bSpawns;
    const Spawn *commonRespawns;
    int32_t numA, numB, numCommon, numDefaultA, numDefaultB;
    int32_t spawnTrackLen; // slots per SpawnUsageCounter list: max(128, longest list)
    mp::AABB zoneAABB[kMaxZones];
    float zoneRot[kMaxZones];
    int32_t numZones;
    int32_t task;           // MPENV_TASK_ZONE or MPENV_TASK_ZONE_CAPTURE_DEFEND
    int32_t flank;          // RewardMode::Flank (train_flank)
    ZOBBDev subZones[8];    // SubZones only (level_gen.cpp:282-326)
    GoalRegionDev goals[4];
    int32_t numGoals;
    uint32_t simFlags;
    int32_t autoReset;
    uint32_t worldOffset;
    mp::RandKey initRandKey;
    // navmesh for the scripted bots (sim.cpp:4958-5172)
    const float *navTris;   // 9 floats per triangle (deduplicated vertices)
    const int32_t *astar;   // [numNavTris][numNavTris] next hop
    const float *navCdf;    // [numNavTris] running triangle areas (NavmeshSpawn)
    // TrajectoryCurriculum (level_gen.cpp:498-581), curriculum_data_path
    const mpenv_curriculum_snapshot *curriculum;
    int32_t numSnapshots;
    int32_t numNavTris;
    // NearestNavTri of each zone's centroid (computed once at scene upload
    // by k_zone_goals with the same device function planAStarD would run)
    int32_t zoneGoalTri[kMaxZones];
    // logs (sim.cpp:4750-4843 record/replay, 23-106 + 4592-4634 events)
    int32_t recordOn, replayOn, eventsOn;
    // Sphere-cast vertex-quirk grid (k_move): bit per qgCell x qgCell cell
    // of the xy plane, set where some BVH vertex lies within
    // agentRadius + 2 of the cell (scene.h quirkGrid); a cast from o can only
    // meet the testVert quirk when the cell of 2o is set.
    const uint32_t *quirkGrid;
    float qgMinX, qgMinY, qgInvCell;
    int32_t qgW, qgH;
};

// Scene residency: the images stageBVHSphere and
// stageBVHOct build, built once in global memory by k_scene_images, and
// which of the two the kernels walk.  Beside SceneDev, not in it: the
// LDS-resident kernels' arguments are what they were, and only the global
// instantiations take this as one more.
enum : int32_t { kResidencyLds = 0, kResidencyGlobal = 1 };
struct SceneImages {
    char *sphere; // geom_dev.h SphereImage (begins with its CollisionImage, which stageBVH views)
    char *oct;    // geom_dev.h OctImage
    int32_t residency;
};

// Host launchers: each in the file of its kernel (move, vis, obs, lidar, hooks;
// k_sim's, the scene upload's and the action kernels' in kernels.hip)
enum KernelId { kKMove = 0, kKSim = 1, kKVis = 2, kKObs = 3, kKLidar = 4, kNumTimedKernels = 5 };

const char *kernelName(int k);
// The images' total bytes (layouts: geom_dev.h CollisionImage, SphereImage, OctImage)
size_t bvhLdsBytes(const SceneDev &sc);
size_t bvhLdsBytesSphere(const SceneDev &sc); // sphere-casting kernels
size_t bvhLdsBytesOct(const SceneDev &sc);    // k_lidar
// The dynamic LDS each step kernel asks for under a residency (only the
// scene's counts are read, so a SceneDev without device pointers will do).
// k_vis's also depends on the team size; T = 0: the largest over all of them.
size_t moveLdsBytes(const SceneDev &sc, int32_t residency);
size_t simLdsBytes(const SceneDev &sc, int32_t residency);
size_t visLdsBytes(const SceneDev &sc, int32_t residency, int T);
size_t lidarLdsBytes(const SceneDev &sc, int32_t residency);
// Fills img.sphere / img.oct; synchronous on `stream`
int buildSceneImages(const SceneDev &sc, const SceneImages &img, void *stream);

int launchConstruct(const DevState &s, const SceneDev &sc, const int32_t ctor_train_ctrl[3], void *stream);
int launchResetOnly(const DevState &s, const SceneDev &sc, void *stream);
int launchMove(const DevState &s, const SceneDev &sc, const SceneImages &img, void *stream);
int launchSimStep(const DevState &s, const SceneDev &sc, const SceneImages &img, void *stream);
int launchVisibility(const DevState &s, const SceneDev &sc, const SceneImages &img, void *stream);
int launchObservations(const DevState &s, const SceneDev &sc, void *stream);
// k_obs over a wire message (wire.hip launchWireUnpack): `view` is the
// shadow's DevState with its input columns pointing into the message.
struct WireObs {
    const uint32_t *packed;  // [A] curPose | tgtPose << 8 | weapon << 16 | flags << 24
    const int32_t *epPrev;   // [W] the previous message's episode counters (the shadow's copy)
    int32_t keyframe;        // a keyframe carries the last-known rows: nothing is cleared
};
int launchObservationsWire(const DevState &view, const SceneDev &sc, const WireObs &wo, void *stream);
// k_lidar: a block's 16 waves share `iters` x 16 wave tasks, 1 <= iters <=
// lidarItersMax(); lidarItersFor is the automatic choice for A agents.
int lidarItersMax();
int lidarItersFor(int64_t A);
int launchLidar(const DevState &s, const SceneDev &sc, const SceneImages &img, int iters, void *stream);
// synchronous on `stream`, at scene upload; dev_scratch holds kMaxZones ints
int computeZoneGoalTris(const SceneDev &sc, int32_t *dev_scratch, int32_t *host_out, void *stream);
int launchTraceRays(const SceneDev &sc, const SceneImages &img, const float *o, const float *d, int n, int mode,
                    float *t, int32_t *hit, void *stream);
// mpenv_debug_geom_queries (include/mpenv.h)
int launchGeomQueries(const SceneDev &sc, const SceneImages &img, int mode, int n, const mpenv_geom_queries &q,
                      void *stream);
int launchDebugGather(const DevState &s, float *af, int32_t *ai, int32_t *wi, float *wf, uint32_t *explore,
                      float *crumbs, void *stream);
int launchFillActions(const DevState &s, const int32_t *src6, void *stream);
int launchCombatActions(const DevState &s, const int32_t *tape6, int32_t *out6, int32_t mode, void *stream);
int computeSceneFrames(SceneTables *d_tab, void *stream); // fills zoneFrame / goalFrame in place

// Batched device copies (wire.hip): up to kMaxCopySegs segments in one
// launch; src == nullptr zero-fills.  Pointers must be 16-B aligned.
constexpr int kMaxCopySegs = 32;
struct CopySeg {
    const void *src;
    void *dst;
    int64_t bytes;
};
struct CopyBatch {
    CopySeg seg[kMaxCopySegs];
    int n;
    int64_t first[kMaxCopySegs + 1]; // first block of each segment (filled by launchCopyBatch)
    // gpuStreamStep's out table rides the copy launches: block 0 stores
    // `tab` to *tabDst (null: nothing), so setting it before the step and
    // clearing it after costs no launch of its own
    OutTab *tabDst;
    OutTab tab;
};
int launchCopyBatch(const CopyBatch &b, void *stream);

// World checkpoints (state.hip; DESIGN.md §3 "World checkpoints").  A
// snapshot is a position-independent byte blob: a 256-B StateHeader, then one
// section per state buffer in declaration order, each at a multiple of 256 B,
// holding that buffer's rows for all worlds in world order (world s's rows
// are one contiguous span of every section).
constexpr uint32_t kStateMagic = 0x3153504du; // "MPS1"
constexpr uint32_t kStateVersion = 1;
constexpr int kMaxStateSegs = 192;

struct StateHeader {
    uint32_t magic, version;
    int32_t W, N, T, spawnTrackLen;
    uint32_t simFlags;
    int32_t task;
    int64_t bytes;
    int32_t sections, pad;
    uint32_t reserved[52];
};
static_assert(sizeof(StateHeader) == 256, "state header");

// One section as mpenv_state_section reports it (host only, no GPU).
struct StateSectionInfo {
    const char *name;  // the export's name without MPENV_EXPORT_, else the DevState member's
    int64_t offset, bytes;
    int32_t rowBytes, rowKind, exportId; // exportId -1: not an export
    int32_t dtype;  // MPENV_DTYPE_* of the elements
    int32_t member; // offsetof(DevState, <member>); dmgCol >= 0: column of dmg
    int32_t dmgCol;
};
int stateNumSections();
// false when idx is out of range
bool stateSection(int idx, int64_t W, int64_t N, int64_t trackLen, StateSectionInfo &out);
int64_t stateBytes(int64_t W, int64_t N, int64_t trackLen);

// The device-resident descriptor table both checkpoint kernels run over,
// built once at create (buildStateTab) and uploaded; segment 0 is the header
// (its live copy is `hdr` below), so a save writes it with the same copy.
struct StateSeg {
    char *live;        // the live buffer (world 0's span)
    int64_t off;       // section offset in the blob
    int64_t bytes;     // W * span
    int32_t span;      // bytes per world
    int32_t gran;      // largest power of two <= 16 dividing span and the live address
};
struct StateTab {
    StateHeader hdr;
    StateSeg seg[kMaxStateSegs];
    // streaming copy (save / full load): first block of each segment, then the total
    int64_t first[kMaxStateSegs + 1];
    // mapped load: the wide sections (a wave per world span; wideBlocks
    // blocks each, in front) and the narrow ones (a lane per element; first
    // block of each, counted from the end of the wide blocks)
    int64_t firstNarrow[kMaxStateSegs + 1];
    int32_t wideSeg[kMaxStateSegs], narrowSeg[kMaxStateSegs];
    int64_t blocks, blocksMap, wideBlocks; // grids of the two kernels; blocks per wide section
    int32_t nSeg, W, nWide, nNarrow;
    uint32_t go;  // written by k_state_check, read by the load that follows it
    uint32_t err; // MPENV_STATE_ERR_* (mpenv_state_error reads and clears)
    // Map sets (mpenv_maps.h): the range of each world (device, [W]) and the
    // scene of each range; k_state_check refuses a world map that takes a
    // world's state from a snapshot world of another scene.  Null for a
    // single-map manager: nothing to check.
    const int32_t *mapOfWorld;
    int32_t rangeScene[MPENV_MAX_MAP_RANGES];
};
// throws std::runtime_error for a section whose buffer is not allocated (a
// table buffer that is neither a section nor exempt fails state.hip's build)
void buildStateTab(const DevState &s, const SceneDev &sc, StateTab *dev, StateTab &host);
int launchStateSave(const StateTab &host, StateTab *dev, char *dst, void *stream);
// map == nullptr: every world from its own snapshot world
int launchStateLoad(const StateTab &host, StateTab *dev, const char *src, const int32_t *map, void *stream);

// Learner-exchange wire format (wire.hip)
int64_t wireBytes(const DevState &s, bool keyframe);
int launchWirePack(const DevState &s, char *dst, bool keyframe, uint32_t worldOffset, void *stream);
// epPrev / epNext: the shadow's double-buffered copies of the previous and
// this message's episode counters ([W] each, swapped by the caller per unpack)
int launchWireErrClear(uint32_t *err, void *stream); // keeps only the desync bit
int launchWireUnpack(const DevState &s, const SceneDev &sc, const char *src, bool keyframe, uint32_t *err,
                     uint32_t worldOffset, const int32_t *epPrev, int32_t *epNext, void *stream);

} // namespace mpenv
