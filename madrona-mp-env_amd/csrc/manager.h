// manager.h — what manager.cpp, manager_scene.cpp, camera.cpp, league.cpp and curriculum.cpp share, and
// nothing else includes: the error channel of the C ABI, the owning HIP handle types and
// struct mpenv_manager.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "camera.h"
#include "curriculum.h"
#include "engine.h"
#include "league.h"
#include "mpenv.h"
#include "policy.h"
#include "scene.h"

using namespace mpenv;

namespace mpenv {
// Sets this thread's mpenv_last_error text and returns `code` (manager.cpp).
int fail(int code, const std::string &msg);
// manager_scene.cpp: which residency a scene can have -- the one place that
// decides it, for mpenv_create, mpenv_set_scene_residency and mpenv_scene_info.
struct SceneLimits {
    int32_t tris = 0, lidarTris = 0, nodes = 0, lidarNodes = 0, stack = 0, lidarStack = 0;
    size_t ldsMove = 0, ldsSim = 0, ldsVis = 0, ldsLidar = 0; // dynamic LDS asked for on the LDS path
    size_t globalBytes = 0;                                     // the global-resident images
    bool ldsOk = false;     // meets every limit of the LDS-resident path
    bool supported = false; // by one path at least
    std::string ldsWhyNot;  // the first LDS limit missed
    std::string reason;     // !supported: why
};
SceneLimits sceneLimits(const Scene &s);
// manager_scene.cpp: a scene's device image (`sc`, `img` and their buffers,
// owned by m) from the loaded scene, its limits and m.cfg.
void buildSceneDev(mpenv_manager &m, const Scene &s, const SceneLimits &limits, SceneDev &sc, SceneImages &img);
// manager_scene.cpp: why cfg's task or flags rule the scene out ("": they do not)
std::string sceneTaskProblem(const Scene &s, const mpenv_config &cfg);

// Scenes and world ranges (mpenv_maps.h; DESIGN.md §2 definition 19).  One
// loaded scene; sc holds the manager's world_id_offset and the largest
// spawnTrackLen of the manager's scenes.
struct MapScene {
    std::string path;
    Scene scene;
    SceneDev sc;
    SceneImages img {};
    SceneLimits limits;
    uint64_t collisionsHash = 0; // FNV-1a 64 of collisions.bin (scene.h)
};
// One range: worlds [w0, w0 + n) as a complete engine (sliceState) on
// scenes[scene].  A manager's `ranges` tile its batch; a world group is a
// sub-range of ranges[0].
struct MapRange {
    int32_t scene = 0, w0 = 0, n = 0;
    DevState S {};
    SceneDev sc {};
};
// manager_scene.cpp: what mpenv_create_maps and mpenv_maps_plan make of a
// list, without a GPU.  Returns MPENV_OK or the refusal's code (its message
// is in mpenv_last_error; `desc`, when not null, is filled as far as the list
// was read).
struct MapPlan {
    std::vector<MapScene> scenes; // loaded, limits set; no device image yet
    std::vector<MapRange> ranges; // scene, w0, n
    int32_t spawnTrackLen = 0;    // the largest of the scenes'
};
int planMaps(const mpenv_config &cfg, const mpenv_map_range *maps, int32_t n, MapPlan &plan, mpenv_map_desc *desc);
} // namespace mpenv

#define HIP_CHECK(expr)                                                                   \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess) {                                                           \
            throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(e_) + \
                                     " at " #expr);                                       \
        }                                                                                 \
    } while (0)

// The result of a launchX() of engine.h: non-zero is a failed launch.
inline void launched(int rc, const char *what)
{
    if (rc) throw std::runtime_error(what);
}

// The body of a C ABI entry point: its return code (MPENV_OK for a body
// that returns nothing), or the code of what it threw -- MPENV_ERR_IO for an
// IoError (scene.h), `other` for any other exception -- with the exception's
// text as mpenv_last_error.
template <class F>
int guarded(F &&body, int other = MPENV_ERR_HIP)
{
    try {
        if constexpr (std::is_void<decltype(body())>::value) {
            body();
            return MPENV_OK;
        } else {
            return body();
        }
    } catch (const IoError &e) {
        return fail(MPENV_ERR_IO, e.what());
    } catch (const std::exception &e) {
        return fail(other, e.what());
    }
}

// One owned HIP handle, released with Drop by the destructor; move-only,
// empty (null) by default and after being moved from into a new Handle.
// Move assignment swaps: the source leaves with the target's previous
// handle and releases it when it dies (every source here is a temporary or
// a local at the end of its scope).  put() is where a HIP create call
// writes the handle: on an empty one only.
template <class T, auto Drop>
class Handle {
public:
    Handle() = default;
    Handle(Handle &&o) noexcept : h_(o.release()) {}
    Handle &operator=(Handle &&o) noexcept { std::swap(h_, o.h_); return *this; }
    ~Handle() { if (h_) (void)Drop(h_); }
    T get() const { return h_; }
    operator T() const { return h_; }
    T *put() { return &h_; }
    T release() { return std::exchange(h_, T {}); } // the caller owns it from here

private:
    T h_ {};
};

inline hipError_t syncAndDestroy(hipStream_t s)
{
    (void)hipStreamSynchronize(s);
    return hipStreamDestroy(s);
}

struct Stream : Handle<hipStream_t, syncAndDestroy> {
    static Stream create(unsigned flags)
    {
        Stream s;
        HIP_CHECK(hipStreamCreateWithFlags(s.put(), flags));
        return s;
    }
};

struct Event : Handle<hipEvent_t, hipEventDestroy> {
    static Event create(unsigned flags)
    {
        Event e;
        HIP_CHECK(hipEventCreateWithFlags(e.put(), flags));
        return e;
    }
};

struct DevPtr : Handle<void *, hipFree> {
    static DevPtr create(size_t bytes)
    {
        DevPtr p;
        HIP_CHECK(hipMalloc(p.put(), bytes));
        return p;
    }
};

// A captured graph and its executable; the executable is destroyed first.
using Graph = Handle<hipGraph_t, hipGraphDestroy>;
struct StepGraph {
    Graph graph;
    Handle<hipGraphExec_t, hipGraphExecDestroy> exec;
};

// A stream beside a main one.  Its work starts after an event the caller
// recorded on the main stream (one fork event may start several side
// streams) and is joined back through `done`.  Both handles or neither.
struct SideStream {
    Stream stream;
    Event done;
    static SideStream create()
    {
        return { Stream::create(hipStreamNonBlocking), Event::create(hipEventDisableTiming) };
    }
    explicit operator bool() const { return stream != nullptr; }
    void startAfter(hipEvent_t recorded) const { HIP_CHECK(hipStreamWaitEvent(stream, recorded, 0)); }
    void markDone() const { HIP_CHECK(hipEventRecord(done, stream)); }
    void joinInto(hipStream_t st) const { HIP_CHECK(hipStreamWaitEvent(st, done, 0)); }
};

struct TensorDesc {
    void *ptr = nullptr;
    int32_t dtype = MPENV_DTYPE_FLOAT32;
    std::vector<int64_t> dims;
    size_t bytes() const
    {
        size_t n = 4;
        for (int64_t d : dims) n *= (size_t)d;
        return n;
    }
};

// Handle members are released in reverse order of declaration: the step
// graph's executable before every stream, the main stream last.
struct mpenv_manager {
    mpenv_config cfg;
    int gpu = 0;
    int32_t residencyMode = MPENV_SCENE_AUTO; // as asked for
    DevState S; // the whole batch: exports, checkpoints, wire, policy, league
    Stream stream;
    std::vector<void *> allocations;
    // The loaded scenes and the world ranges that tile the batch: one of
    // each, {scene 0, world 0, W}, from mpenv_create; the planned list from
    // mpenv_create_maps.  The step, the init, the construct and the camera
    // loop over `ranges` in order on the call's stream.  A scene's img (the
    // residency in use) is part of the step graph's key.
    std::vector<MapScene> scenes;
    std::vector<MapRange> ranges;
    // range 0's scene: what the ray and geometry test hooks, the wire calls,
    // the log flags and the buffer table's trackLen read
    MapScene &firstScene() { return scenes[ranges[0].scene]; }
    int32_t *mapOfWorld = nullptr; // device [W]: range index per world (mpenv_map_of_world)
    // created from a list (of one range or more): what the refusals, the
    // checkpoint header's layout hash and the env overrides at create go by
    bool fromList = false;
    bool mapSet() const { return fromList; }

    // Debug gather buffers (allocated lazily)
    float *dbgAF = nullptr, *dbgWF = nullptr, *dbgCrumbs = nullptr;
    int32_t *dbgAI = nullptr, *dbgWI = nullptr;
    uint32_t *dbgExplore = nullptr;

    // World groups: ranges[0] cut into contiguous sub-ranges (groupRanges;
    // none for one group) stepped on their own streams (fork/join with
    // events) so independent kernels overlap on the GPU.  One fork event
    // starts every group; group 0 runs on the caller's stream, group i > 0
    // on gside[i - 1].
    int groups = 1;
    std::vector<SideStream> gside;
    std::vector<MapRange> groupRanges;
    Event forkEv;
    // One group only: k_lidar on a branch stream beside k_vis -> k_obs (no
    // data dependence between them after k_sim).  MPENV_LIDAR_BRANCH=1.
    bool lidarBranch = false;
    SideStream bSide;
    Event bForkEv;
    // k_lidar's tasks per wave: 0 = lidarItersFor(agents of the range), else
    // forced (mpenv_set_lidar_iters)
    int lidarIters = 0;
    int lidarItersOf(const DevState &R) const { return lidarIters ? lidarIters : lidarItersFor(R.A); }
    // gpuStreamStep: the agent maps' zero fills (no dependence on the step)
    // on a side stream of their own, overlapping the step's kernels; joined
    // back into the caller's stream before the call returns.
    SideStream zSide;
    Event zForkEv;

    // Record / replay / event logs (mgr.cpp:155-300: per-step file I/O
    // around the Step graph)
    FILE *replayFile = nullptr, *recordFile = nullptr, *eventsFile = nullptr, *stepsFile = nullptr;
    bool replayEof = false;
    std::vector<mpenv_step_log> hostLog;
    std::vector<mpenv_game_event> hostEvents;
    std::vector<mpenv_packed_step_snapshot> hostSnaps;
    std::vector<int32_t> hostSnapWritten;

    // Workload counters (DevState::stats, kNumStats u64), allocated on first use
    unsigned long long *statsBuf = nullptr;

    // Kernel timing
    bool timing = false;
    std::vector<Event> eventPool;
    size_t eventsUsed = 0;

    // The Step graph as a captured HIP graph (all world groups, fork/join
    // included), replayed with one hipGraphLaunch per step.  Kernel
    // arguments are captured by value, so the graph is keyed on the bytes of
    // every argument struct and re-captured when any of them changes (world
    // groups, stats buffer, ...).  MPENV_STEP_GRAPH=0 launches kernel by
    // kernel instead; timed steps (events between kernels) always do.
    bool useGraph = true;
    Stream capStream;
    StepGraph step;
    std::vector<char> graphKey;
    // recorded after every hipGraphLaunch on the launch's stream: a
    // re-capture waits on it before destroying the previous exec (its last
    // launch may still run on a caller stream the manager does not own)
    Event graphDoneEv;
    int64_t graphCaptures = 0; // mpenv_graph_captures
    std::string graphOffReason; // why the step is not replayed from a graph (mpenv_graph_status)
    uint32_t *wireErr = nullptr; // device word raised by a rejected wire message (wire.hip)
    int32_t *wireEp = nullptr;   // [2][W] a shadow's episode counters of the last two messages
    int wireParity = 0;          // which half of wireEp holds the previous message's
    OutTab *outTabDev = nullptr; // gpuStreamStep's caller output buffers (engine.h OutTab)
    // World checkpoints (state.hip): the descriptor table, its device copy,
    // and which log mode (append-only files) rules them out for this manager
    StateTab stateTab;
    StateTab *stateTabDev = nullptr;
    const char *stateRefused = nullptr;
    // In-sim policy inference (policy.hip; DESIGN.md §2 definition 15): the
    // one parameter blob per occupied checkpoint slot (polBlobs, the host's
    // copy of the device table polDev.blobs; polDev.mask says which); the
    // table and the work buffers live from the first load to the last
    // unload; while any slot is occupied (polLoaded), every step first
    // writes the served agents' actions
    PolicyDev polDev {};
    const float *polBlobs[pol::kSlots] = {};
    int32_t *polTab = nullptr; // the allocation behind polDev's counters and tile tables
    bool polLoaded = false;
    int32_t polPrecision = MPENV_POLICY_F32; // which trunk kernel runs (definition 15 or 16); every blob serves both
    // the last step was a gpuStreamStep that wrote the observation rows into
    // its caller's buffers only (OutTab): the engine's own rows, which the
    // policy, the aim-bot (mpenv_combat_actions) and a snapshot
    // (mpenv_state_save) read, are behind until a plain step, a copying
    // gpuStreamStep or an init writes them again; those three calls are
    // refused meanwhile (staleExports)
    bool exportsStale = false;
    // The egocentric camera (camera.cpp, mpenv_camera.h; DESIGN.md §2
    // definition 18): one allocation for both images and the ray tables.
    // While on, every step and init is followed by k_camera on its stream,
    // outside the captured graph; no part of the state, the snapshots, the
    // wire format or the graph's key.
    bool camOn = false;
    mpenv_camera_config camCfg {};
    CameraDev cam {};
    DevPtr camBuf;
    // The league scheduler (league.cpp, mpenv_league.h; DESIGN.md §2
    // definition 20): one allocation for the standings table, the weights
    // and the draw counters.  While on, every step and init is followed by
    // k_league on its stream, outside the captured graph; no part of the
    // state, the snapshots, the wire format or the graph's key.
    bool leagueOn = false;
    mpenv_league_config leagueCfg {};
    LeagueDev league {};
    DevPtr leagueBuf;
    // The live curriculum pool (curriculum.cpp, mpenv_curriculum.h; DESIGN.md
    // §2 definition 21): one allocation for the snapshots, their ticks and
    // the range table.  While on, every range's (and group's) sc.curriculum
    // points into it -- scenes[].sc keeps what creation set, which disable
    // restores -- and every step is followed by k_harvest on its stream,
    // outside the captured graph.  No part of the state, the snapshots or the
    // wire format.  `inited`: an init has run (the pool is filled from the batch).
    bool inited = false;
    bool poolOn = false;
    mpenv_curriculum_pool_config poolCfg {};
    PoolDev pool {};
    DevPtr poolBuf;
    uint32_t poolTick = 0; // harvests since enable

    ~mpenv_manager();

    template <typename T>
    T *alloc(size_t count)
    {
        size_t bytes = std::max<size_t>(count * sizeof(T), 16);
        void *p = nullptr;
        HIP_CHECK(hipMalloc(&p, bytes));
        HIP_CHECK(hipMemsetAsync(p, 0, bytes, stream));
        allocations.push_back(p);
        return static_cast<T *>(p);
    }

    // Host->device copy ordered on the manager stream (after the zeroing
    // memsets issued by alloc() and any in-flight step), then waited for.
    void upload(void *dst, const void *src, size_t bytes)
    {
        HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
    }

    void freePolicy();
    void allocPolicyWork();
    void setPolicySlot(int slot, const float *blob);
    void record(hipStream_t st);
    void stepRange(const MapRange &r, hipStream_t st);
    void preStep(hipStream_t st);
    void postStep(hipStream_t st);
    void runStep(hipStream_t st);
    std::vector<char> argKey() const;
    void launchStep(hipStream_t st);
    bool captureStep();
    void launchStepDirect(hipStream_t st);
    void setupGroups(int want);
    void setStats(unsigned long long *p);
    void runInitGraph(hipStream_t st);
    void renderCamera(hipStream_t st); // camera.cpp
    void runLeague(hipStream_t st, bool initOnly); // league.cpp
    void runHarvest(hipStream_t st); // curriculum.cpp
    bool exportDesc(int32_t id, TensorDesc &d);
    void *exportPtr(int32_t id);
    void gatherDebug(bool explore = false);
};

// The caller's stream of an entry point, or the manager's own for null.
inline hipStream_t streamOf(const mpenv_manager *m, void *stream)
{
    return stream ? (hipStream_t)stream : (hipStream_t)m->stream;
}
