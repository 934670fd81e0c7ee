// manager.cpp — the Manager (src/mgr.hpp:31-161, src/mgr.cpp) for the gfx950
// engine, exposed through the C ABI of include/mpenv.h.
//
// Owns every device buffer (engine-owned tensors, zero-copy views handed to
// callers as in mgr.cpp:295-301/655-661), the scene upload (manager_scene.cpp)
// and the step launch sequence on a HIP stream; the struct and its owning
// handles are in manager.h.  There is no CPU execution path: a CPU ExecMode is
// rejected (the reference's CPU TaskGraph executor is restated only by the
// test oracle).
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <unordered_set>

#include <dlfcn.h>

#include "manager.h"

static thread_local std::string g_last_error;

int mpenv::fail(int code, const std::string &msg)
{
    g_last_error = msg;
    return code;
}

namespace {

// Order of TrainInterface inputs/outputs (mgr.cpp:2383-2431).  An output
// with `direct` set is one gpuStreamStep has k_obs / k_lidar write straight
// into the caller's buffer, through that member of OutTab (engine.h),
// instead of copying it afterwards.  `zero` marks the agent maps: the step
// never writes them and they stay all zeros, so their copy is a zero fill
// (on the direct path k_lidar's, through the table).
struct TIEntry {
    const char *name;
    int32_t id;
    float *OutTab::*direct = nullptr;
    bool zero = false;
};
const TIEntry kTIInputs[] = {
    { "discrete", MPENV_EXPORT_PVP_DISCRETE_ACTION },
    { "aim", MPENV_EXPORT_PVP_DISCRETE_AIM_ACTION },
    { "resets", MPENV_EXPORT_RESET },
    { "simCtrl", MPENV_EXPORT_SIM_CONTROL },
    { "pbt.policy_assignments", MPENV_EXPORT_AGENT_POLICY },
};
const TIEntry kTIOutputs[] = {
    { "fwd_lidar", MPENV_EXPORT_FWD_LIDAR, &OutTab::fwdLidar },
    { "rear_lidar", MPENV_EXPORT_REAR_LIDAR, &OutTab::rearLidar },
    { "hp", MPENV_EXPORT_HP },
    { "magazine", MPENV_EXPORT_MAGAZINE },
    { "alive", MPENV_EXPORT_ALIVE },
    { "self", MPENV_EXPORT_SELF_OBSERVATION, &OutTab::selfObs },
    { "filters_state", MPENV_EXPORT_FILTERS_STATE, &OutTab::filters },
    { "teammates", MPENV_EXPORT_TEAMMATE_OBSERVATIONS, &OutTab::tmObs },
    { "opponents", MPENV_EXPORT_OPPONENT_OBSERVATIONS, &OutTab::oppObs },
    { "opponents_last_known", MPENV_EXPORT_OPPONENT_LAST_KNOWN_OBSERVATIONS },
    { "self_pos", MPENV_EXPORT_SELF_POSITION, &OutTab::selfPos },
    { "teammate_positions", MPENV_EXPORT_TEAMMATE_POSITIONS, &OutTab::tmPos },
    { "opponent_positions", MPENV_EXPORT_OPPONENT_POSITIONS, &OutTab::oppPos },
    { "opponent_last_known_positions", MPENV_EXPORT_OPPONENT_LAST_KNOWN_POSITIONS },
    { "opponent_masks", MPENV_EXPORT_OPPONENT_MASKS, &OutTab::masks },
    { "agent_map", MPENV_EXPORT_AGENT_MAP, &OutTab::agentMap0, true },
    { "unmasked_agent_map", MPENV_EXPORT_AGENT_MAP, &OutTab::agentMap1, true },
    { "reward_coefs", MPENV_EXPORT_REWARD_HYPER_PARAMS },
    { "rewards", MPENV_EXPORT_REWARD },
    { "dones", MPENV_EXPORT_DONE },
    { "pbt.episode_results", MPENV_EXPORT_MATCH_RESULT },
};
constexpr int kNumTIInputs = sizeof(kTIInputs) / sizeof(kTIInputs[0]);
constexpr int kNumTIOutputs = sizeof(kTIOutputs) / sizeof(kTIOutputs[0]);

} // namespace

void mpenv_manager::freePolicy()
{
    polLoaded = false;
    for (const float *&b : polBlobs) {
        if (b) (void)hipFree((void *)b);
        b = nullptr;
    }
    for (void *p : { (void *)polDev.blobs, (void *)polDev.emb, (void *)polDev.list, (void *)polTab })
        if (p) (void)hipFree(p);
    polDev = PolicyDev {};
    polTab = nullptr;
}

// The slot table (all empty), the list, the embeddings and the selection's
// counters and tile tables (policy.h), zeroed: the first load.
void mpenv_manager::allocPolicyWork()
{
    auto dev = [&](size_t bytes) {
        void *p = nullptr;
        HIP_CHECK(hipMalloc(&p, bytes));
        HIP_CHECK(hipMemsetAsync(p, 0, bytes, stream));
        return p;
    };
    const int64_t rows = pol::listRows(S.A);
    polDev.blobs = static_cast<const float *const *>(dev(pol::kSlots * sizeof(float *)));
    polDev.emb = static_cast<float *>(dev((size_t)rows * pol::kTrunkIn * sizeof(float)));
    polDev.list = static_cast<int32_t *>(dev((size_t)rows * sizeof(int32_t)));
    polTab = static_cast<int32_t *>(dev((size_t)pol::tabBytes(S.A)));
    polDev.count = polTab;
    polDev.cursor = polTab + pol::kSlots;
    polDev.tiles = reinterpret_cast<pol::Tile *>(polTab + 2 * pol::kSlots);
    HIP_CHECK(hipStreamSynchronize(stream));
}

// Slot `slot` holds `blob` (device memory, owned from here on) or, null,
// nothing; the old blob is freed.  The caller has waited for whatever may
// still read the table or the old blob.
void mpenv_manager::setPolicySlot(int slot, const float *blob)
{
    // the last selection's tiles name blobs as they were: every tile dies here (rows = 0), so
    // the trunk alone (mpenv_debug_policy_step) never follows one to a freed blob
    HIP_CHECK(hipMemsetAsync(polTab, 0, (size_t)pol::tabBytes(S.A), stream));
    upload((void *)(polDev.blobs + slot), &blob, sizeof(blob));
    if (polBlobs[slot]) (void)hipFree((void *)polBlobs[slot]);
    polBlobs[slot] = blob;
    polDev.mask = blob ? polDev.mask | (1u << slot) : polDev.mask & ~(1u << slot);
    polLoaded = polDev.mask != 0;
}

mpenv_manager::~mpenv_manager()
{
    // nothing may still run when the device memory goes; the handles are
    // released by their members afterwards
    if (stream) (void)hipStreamSynchronize(stream);
    for (const SideStream &g : gside) (void)hipStreamSynchronize(g.stream);
    for (const SideStream *s : { &bSide, &zSide })
        if (*s) (void)hipStreamSynchronize(s->stream);
    if (graphDoneEv) (void)hipEventSynchronize(graphDoneEv);
    for (FILE *f : { replayFile, recordFile, eventsFile, stepsFile })
        if (f) std::fclose(f);
    for (void *p : allocations) (void)hipFree(p);
    freePolicy();
}

// Kernel timing: the next event of the pool (grown on demand) recorded on st.
void mpenv_manager::record(hipStream_t st)
{
    if (!timing) return;
    if (eventsUsed == eventPool.size()) eventPool.push_back(Event::create(hipEventDefault));
    HIP_CHECK(hipEventRecord(eventPool[eventsUsed++], st));
}

// The Step graph over one world range on one stream.  With timing on,
// kNumTimedKernels + 1 events bracket the kernels (one segment per
// range per step, contiguous in the pool).
void mpenv_manager::stepRange(const MapRange &r, hipStream_t st)
{
    const DevState &R = r.S;
    const SceneDev &rsc = r.sc;
    const SceneImages &img = scenes[r.scene].img;
    record(st);
    launched(launchMove(R, rsc, img, st), "k_move launch failed");
    record(st);
    launched(launchSimStep(R, rsc, img, st), "k_sim launch failed");
    record(st);
    if (lidarBranch && groups == 1 && !timing && !mapSet()) {
        HIP_CHECK(hipEventRecord(bForkEv, st));
        bSide.startAfter(bForkEv);
        launched(launchLidar(R, rsc, img, lidarItersOf(R), bSide.stream), "k_lidar launch failed");
        bSide.markDone();
        launched(launchVisibility(R, rsc, img, st), "k_vis launch failed");
        launched(launchObservations(R, rsc, st), "k_obs launch failed");
        bSide.joinInto(st);
        return;
    }
    launched(launchVisibility(R, rsc, img, st), "k_vis launch failed");
    record(st);
    launched(launchObservations(R, rsc, st), "k_obs launch failed");
    record(st);
    launched(launchLidar(R, rsc, img, lidarItersOf(R), st), "k_lidar launch failed");
    record(st);
}

// Replay: next W StepLogs from the file (a short read at EOF keeps the
// rest of the previous step's records, as the reference's fstream read).
void mpenv_manager::preStep(hipStream_t st)
{
    if (!replayFile) return;
    const size_t n = std::fread(hostLog.data(), sizeof(mpenv_step_log), hostLog.size(), replayFile);
    if (n < hostLog.size()) replayEof = true;
    HIP_CHECK(hipMemcpyAsync((void *)S.replayLog, hostLog.data(), sizeof(mpenv_step_log) * hostLog.size(),
                             hipMemcpyHostToDevice, st));
}

// Record: W StepLogs per step.  Events: the step's events world-major
// (per world: agent slots in order, then the capture) to events.bin and
// the written snapshots to steps.bin (writeGameEvents, mgr.cpp:104-116).
void mpenv_manager::postStep(hipStream_t st)
{
    if (!recordFile && !eventsFile) return;
    HIP_CHECK(hipStreamSynchronize(st));
    if (recordFile) {
        HIP_CHECK(hipMemcpy(hostLog.data(), S.recordLog, sizeof(mpenv_step_log) * hostLog.size(),
                            hipMemcpyDeviceToHost));
        std::fwrite(hostLog.data(), sizeof(mpenv_step_log), hostLog.size(), recordFile);
    }
    if (eventsFile) {
        HIP_CHECK(hipMemcpy(hostEvents.data(), S.events, sizeof(mpenv_game_event) * hostEvents.size(),
                            hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(hostSnaps.data(), S.snapshots, sizeof(mpenv_packed_step_snapshot) * hostSnaps.size(),
                            hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(hostSnapWritten.data(), S.snapWritten, sizeof(int32_t) * hostSnapWritten.size(),
                            hipMemcpyDeviceToHost));
        for (const mpenv_game_event &e : hostEvents)
            if (e.type != 0) std::fwrite(&e, sizeof(e), 1, eventsFile);
        for (size_t w = 0; w < hostSnaps.size(); w++)
            if (hostSnapWritten[w]) std::fwrite(&hostSnaps[w], sizeof(hostSnaps[w]), 1, stepsFile);
    }
}

void mpenv_manager::runStep(hipStream_t st)
{
    // evalAgentPolicy runs ahead of the game systems (sim.cpp:5361-5365);
    // in front of the captured graph, which a load or unload leaves alone
    if (polLoaded) launched(launchPolicyStep(S, polDev, st, kPolicyAll, polPrecision), "policy launch failed");
    preStep(st);
    launchStep(st);
    // the camera's images of the state the step left (after the world
    // groups' join, over the whole batch); behind the captured graph, which
    // enabling or disabling a camera leaves alone
    if (camOn) renderCamera(st);
    // the league's standings and redraws for the worlds the step ended: one
    // launch over the whole batch, behind the graph as the camera is
    if (leagueOn) runLeague(st, false);
    // the curriculum pool's refresh from the state the step left: one launch
    // over the pool's slots, behind the graph as well
    if (poolOn) runHarvest(st);
    postStep(st);
}

std::vector<char> mpenv_manager::argKey() const
{
    std::vector<char> k;
    auto put = [&](const void *p, size_t n) {
        const char *c = static_cast<const char *>(p);
        k.insert(k.end(), c, c + n);
    };
    put(&groups, sizeof(groups));
    put(&lidarBranch, sizeof(lidarBranch));
    put(&lidarIters, sizeof(lidarIters));
    // the three structs every stepRange launches with
    for (const std::vector<MapRange> *v : { &ranges, &groupRanges })
        for (const MapRange &r : *v) {
            put(&r.S, sizeof(r.S));
            put(&r.sc, sizeof(r.sc));
            put(&scenes[r.scene].img, sizeof(SceneImages));
        }
    return k;
}

void mpenv_manager::launchStep(hipStream_t st)
{
    if (!useGraph || timing) {
        launchStepDirect(st);
        return;
    }
    std::vector<char> key = argKey();
    if (!step.exec || key != graphKey) {
        if (graphDoneEv) HIP_CHECK(hipEventSynchronize(graphDoneEv));
        step = StepGraph {};
        if (!capStream) capStream = Stream::create(hipStreamNonBlocking);
        // capture on a private stream (the caller's may be the legacy
        // default stream, which cannot be captured); the group streams
        // join the capture through the fork event
        if (!captureStep()) {
            // abandoned capture: this and later steps launch directly
            launchStepDirect(st);
            return;
        }
        graphKey = std::move(key);
        graphCaptures++;
    }
    HIP_CHECK(hipGraphLaunch(step.exec, st));
    if (!graphDoneEv) graphDoneEv = Event::create(hipEventDisableTiming);
    HIP_CHECK(hipEventRecord(graphDoneEv, st));
}

// Captures the Step graph into `step`.  Every capture call
// is checked, and so is the capture's state before it ends (an enqueue
// that invalidated it, a fork not joined back): on any failure the
// capture is ended and discarded, the graph is switched off with the
// reason kept (mpenv_graph_status), and false is returned -- a bad
// capture is never instantiated or launched.
bool mpenv_manager::captureStep()
{
    auto abandon = [&](const std::string &why) {
        Graph g; // of a capture still open: ended and dropped here
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(capStream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
            (void)hipStreamEndCapture(capStream, g.put());
        g = Graph {};
        step = StepGraph {};
        (void)hipGetLastError(); // clear the sticky launch error of a failed capture call
        useGraph = false;
        graphOffReason = why;
        std::fprintf(stderr, "mpenv: step graph off (%s); launching kernels directly\n", why.c_str());
        return false;
    };
    hipError_t e = hipStreamBeginCapture(capStream, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) return abandon(std::string("hipStreamBeginCapture: ") + hipGetErrorString(e));
    try {
        launchStepDirect(capStream);
    } catch (const std::exception &ex) {
        return abandon(std::string("enqueue during capture: ") + ex.what());
    }
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    unsigned long long id = 0;
    e = hipStreamGetCaptureInfo(capStream, &cs, &id);
    if (e != hipSuccess) return abandon(std::string("hipStreamGetCaptureInfo: ") + hipGetErrorString(e));
    if (cs != hipStreamCaptureStatusActive) return abandon("capture invalidated before its end");
    e = hipStreamEndCapture(capStream, step.graph.put());
    if (e != hipSuccess || !step.graph) return abandon(std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    e = hipGraphInstantiate(step.exec.put(), step.graph, nullptr, nullptr, 0);
    if (e != hipSuccess || !step.exec) return abandon(std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
    return true;
}

void mpenv_manager::launchStepDirect(hipStream_t st)
{
    if (groups <= 1) {
        // in range order on the one stream
        for (const MapRange &r : ranges) stepRange(r, st);
        return;
    }
    // group 0 runs on the caller's stream itself, so G groups occupy G
    // hardware queues (GPU_MAX_HW_QUEUES is 4 per process by default)
    HIP_CHECK(hipEventRecord(forkEv, st));
    for (const SideStream &g : gside) g.startAfter(forkEv);
    for (int i = 1; i < groups; i++) {
        stepRange(groupRanges[i], gside[i - 1].stream);
        gside[i - 1].markDone();
    }
    stepRange(groupRanges[0], st);
    for (const SideStream &g : gside) g.joinInto(st);
}

void mpenv_manager::runInitGraph(hipStream_t st)
{
    // triggerReset on every world (mgr.cpp:1936-1938) then the Init graph
    // (sim.cpp:5322-5340): resetSystem + observations + lidar.
    HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)S.reset, 1, (size_t)S.W, st));
    for (const MapRange &r : ranges) {
        const SceneImages &rimg = scenes[r.scene].img;
        launched(launchResetOnly(r.S, r.sc, st), "k_reset launch failed");
        launched(launchVisibility(r.S, r.sc, rimg, st), "k_vis launch failed");
        launched(launchObservations(r.S, r.sc, st), "k_obs launch failed");
        launched(launchLidar(r.S, r.sc, rimg, lidarItersOf(r.S), st), "k_lidar launch failed");
    }
    if (camOn) renderCamera(st);
    if (leagueOn) runLeague(st, true); // every world draws, none is recorded
    inited = true;
}

template <typename T>
constexpr int32_t dtypeOf()
{
    static_assert(std::is_same<T, float>::value || std::is_same<T, int32_t>::value || std::is_same<T, uint32_t>::value,
                  "no MPENV_DTYPE_* for this element type");
    return std::is_same<T, float>::value ? MPENV_DTYPE_FLOAT32
           : std::is_same<T, int32_t>::value ? MPENV_DTYPE_INT32
                                             : MPENV_DTYPE_UINT32;
}

// dtype and dims of an export for W worlds of N agents: no manager, no GPU
// (mpenv_export_layout).  The buffer table's exports, then the ones that
// are not a plain view of a table buffer.
static bool exportLayout(int32_t id, int64_t W, int64_t N, TensorDesc &d)
{
    const int64_t A = W * N;
    auto set = [&](int32_t dt, std::initializer_list<int64_t> dims) {
        d.dtype = dt;
        d.dims.assign(dims.begin(), dims.end());
        return true;
    };
    switch (id) {
#define MP_LAYOUT(n, type, kind, eid, ...) \
    case eid: return set(dtypeOf<type>(), { bufRows(kind, W, N), __VA_ARGS__ });
        MP_BUFS(MP_BUF_SKIP, MP_LAYOUT)
#undef MP_LAYOUT
    case MPENV_EXPORT_UNMASKED_AGENT_MAP: return exportLayout(MPENV_EXPORT_AGENT_MAP, W, N, d);
    case MPENV_EXPORT_EVENT_LOG: return set(MPENV_DTYPE_INT32, { W, 2 * N + 1, 6 });
    case MPENV_EXPORT_PACKED_STEP_SNAPSHOT: return set(MPENV_DTYPE_INT32, { W, 48 });
    case MPENV_EXPORT_RECORD_LOG:
    case MPENV_EXPORT_REPLAY_LOG: return set(MPENV_DTYPE_INT32, { W, 217 });
    case MPENV_EXPORT_SNAPSHOT_WRITTEN: return set(MPENV_DTYPE_INT32, { W, 1 });
    case MPENV_EXPORT_SIM_CONTROL: return set(MPENV_DTYPE_INT32, { 3 });
    case MPENV_EXPORT_DEBUG_AGENT_F32: return set(MPENV_DTYPE_FLOAT32, { A, MPENV_DBG_AF_COUNT });
    case MPENV_EXPORT_DEBUG_AGENT_I32: return set(MPENV_DTYPE_INT32, { A, MPENV_DBG_AI_COUNT });
    case MPENV_EXPORT_DEBUG_WORLD_I32: return set(MPENV_DTYPE_INT32, { W, MPENV_DBG_WI_COUNT });
    case MPENV_EXPORT_DEBUG_WORLD_F32: return set(MPENV_DTYPE_FLOAT32, { W, MPENV_DBG_WF_COUNT });
    case MPENV_EXPORT_DEBUG_EXPLORE: return set(MPENV_DTYPE_UINT32, { A, kGridCells });
    case MPENV_EXPORT_DEBUG_CRUMBS: return set(MPENV_DTYPE_FLOAT32, { W, kMaxCrumbs, 8 });
    default: return false;
    }
}

// The buffer behind an export; null for a log buffer that is not allocated.
void *mpenv_manager::exportPtr(int32_t id)
{
    switch (id) {
#define MP_PTR(n, type, kind, eid, ...) \
    case eid: return S.n;
        MP_BUFS(MP_BUF_SKIP, MP_PTR)
#undef MP_PTR
    case MPENV_EXPORT_UNMASKED_AGENT_MAP: return S.agentMap;
    case MPENV_EXPORT_EVENT_LOG: return S.events;
    case MPENV_EXPORT_PACKED_STEP_SNAPSHOT: return S.snapshots;
    case MPENV_EXPORT_RECORD_LOG: return S.recordLog;
    case MPENV_EXPORT_REPLAY_LOG: return const_cast<mpenv_step_log *>(S.replayLog);
    case MPENV_EXPORT_SNAPSHOT_WRITTEN: return S.snapshots ? S.snapWritten : nullptr;
    case MPENV_EXPORT_SIM_CONTROL: return S.trainCtrl;
    case MPENV_EXPORT_DEBUG_AGENT_F32: gatherDebug(); return dbgAF;
    case MPENV_EXPORT_DEBUG_AGENT_I32: gatherDebug(); return dbgAI;
    case MPENV_EXPORT_DEBUG_WORLD_I32: gatherDebug(); return dbgWI;
    case MPENV_EXPORT_DEBUG_WORLD_F32: gatherDebug(); return dbgWF;
    case MPENV_EXPORT_DEBUG_EXPLORE: gatherDebug(true); return dbgExplore;
    case MPENV_EXPORT_DEBUG_CRUMBS: gatherDebug(); return dbgCrumbs;
    default: return nullptr;
    }
}

bool mpenv_manager::exportDesc(int32_t id, TensorDesc &d)
{
    if (!exportLayout(id, S.W, S.N, d)) return false;
    d.ptr = exportPtr(id);
    return d.ptr != nullptr;
}

void mpenv_manager::gatherDebug(bool explore)
{
    if (!dbgAF) {
        dbgAF = alloc<float>((size_t)S.A * MPENV_DBG_AF_COUNT);
        dbgAI = alloc<int32_t>((size_t)S.A * MPENV_DBG_AI_COUNT);
        dbgWI = alloc<int32_t>((size_t)S.W * MPENV_DBG_WI_COUNT);
        dbgWF = alloc<float>((size_t)S.W * MPENV_DBG_WF_COUNT);
        dbgCrumbs = alloc<float>((size_t)S.W * kMaxCrumbs * 8);
    }
    // the expanded explore grid (4 B per cell, 26 KB per agent) only on request
    if (explore && !dbgExplore) dbgExplore = alloc<uint32_t>((size_t)S.A * kGridCells);
    launched(launchDebugGather(S, dbgAF, dbgAI, dbgWI, dbgWF, explore ? dbgExplore : nullptr, dbgCrumbs, stream),
             "debug gather launch failed");
    HIP_CHECK(hipStreamSynchronize(stream));
}

static void allocState(mpenv_manager &m)
{
    DevState &S = m.S;
    const size_t A = (size_t)S.A, W = (size_t)S.W;
#define MP_ALLOC_AF(n) S.n = m.alloc<float>(A);
#define MP_ALLOC_AI(n) S.n = m.alloc<int32_t>(A);
#define MP_ALLOC_WI(n) S.n = m.alloc<int32_t>(W);
#define MP_ALLOC_WF(n) S.n = m.alloc<float>(W);
    MP_AGENT_F32(MP_ALLOC_AF)
    MP_AGENT_I32(MP_ALLOC_AI)
    MP_WORLD_I32(MP_ALLOC_WI)
    MP_WORLD_F32(MP_ALLOC_WF)
#undef MP_ALLOC_AF
#undef MP_ALLOC_AI
#undef MP_ALLOC_WI
#undef MP_ALLOC_WF
    // T and trackLen: the run-time row shapes of the buffer table (engine.h)
    const int64_t T = S.T, trackLen = m.firstScene().sc.spawnTrackLen;
#define MP_ALLOC(n, type, kind, ...) S.n = m.alloc<type>((size_t)(bufRows(kind, S.W, S.N) * rowElems(__VA_ARGS__)));
#define MP_ALLOC_E(n, type, kind, id, ...) MP_ALLOC(n, type, kind, __VA_ARGS__)
    S.dmg = m.alloc<float>(A * kMaxTeamSize);
    S.dmgStride = (int64_t)A;
    MP_BUFS_A(MP_ALLOC, MP_ALLOC_E)
    m.wireErr = m.alloc<uint32_t>(1);
    HIP_CHECK(hipMemsetAsync(m.wireErr, 0, sizeof(uint32_t), m.stream));
    m.outTabDev = m.alloc<OutTab>(1); // zeros: off
    S.outTab = m.outTabDev;
    m.wireEp = m.alloc<int32_t>(2 * W);
    HIP_CHECK(hipMemsetAsync(m.wireEp, 0, sizeof(int32_t) * 2 * W, m.stream));
    MP_BUFS_B(MP_ALLOC, MP_ALLOC_E)
    HIP_CHECK(hipMemsetAsync(S.visOcc, 0xff, sizeof(uint16_t) * A * T * 4, m.stream)); // hints: none
    S.resetKeys = m.alloc<mp::RandKey>(A * 11);
    MP_BUFS_C(MP_ALLOC, MP_ALLOC_E)
#undef MP_ALLOC
#undef MP_ALLOC_E
    // a buffer the lists above missed would be a null pointer in a kernel
#define MP_NAMED(n, ...) { #n, S.n },
    const struct {
        const char *name;
        const void *ptr;
    } bufs[] = { MP_BUFS(MP_NAMED, MP_NAMED) { "dmg", S.dmg }, { "resetKeys", S.resetKeys } };
#undef MP_NAMED
    for (const auto &b : bufs)
        if (!b.ptr) throw std::runtime_error(std::string("device buffer ") + b.name + " was not allocated");
}

// The log flags go into the scene's SceneDev: before any range or group is
// cut from it.
static void openLogs(mpenv_manager &m, const mpenv_config *cfg)
{
    DevState &S = m.S;
    SceneDev &sc = m.firstScene().sc;
    const size_t W = (size_t)S.W;
    S.evStride = 2 * S.N + 1;
    if (cfg->replay_log_path) {
        m.replayFile = std::fopen(cfg->replay_log_path, "rb");
        if (!m.replayFile) throw IoError(std::string("cannot open replay log ") + cfg->replay_log_path);
        S.replayLog = m.alloc<mpenv_step_log>(W);
        sc.replayOn = 1;
    }
    if (cfg->record_log_path) {
        m.recordFile = std::fopen(cfg->record_log_path, "wb");
        if (!m.recordFile) throw IoError(std::string("cannot open record log ") + cfg->record_log_path);
        S.recordLog = m.alloc<mpenv_step_log>(W);
        sc.recordOn = 1;
    }
    if (m.replayFile || m.recordFile) m.hostLog.assign(W, mpenv_step_log {});
    if (cfg->event_log_path) {
        const std::string dir = cfg->event_log_path;
        m.eventsFile = std::fopen((dir + "/events.bin").c_str(), "wb");
        m.stepsFile = std::fopen((dir + "/steps.bin").c_str(), "wb");
        if (!m.eventsFile || !m.stepsFile) throw IoError("cannot open event logs in " + dir);
        S.events = m.alloc<mpenv_game_event>(W * S.evStride);
        S.snapshots = m.alloc<mpenv_packed_step_snapshot>(W);
        m.hostEvents.assign(W * S.evStride, mpenv_game_event {});
        m.hostSnaps.assign(W, mpenv_packed_step_snapshot {});
        m.hostSnapWritten.assign(W, 0);
        sc.eventsOn = 1;
    }
}

// A contiguous world range [w0, w0 + nw) of the manager viewed as a complete
// engine: every per-agent / per-world column offset to the range, W/A set
// to its size, and the scene's world-id offset advanced so RNG keys stay
// global.  Worlds never read each other, so step kernels launched on
// different ranges are independent and can run on concurrent streams.
static void sliceState(const DevState &S, const SceneDev &sc, int64_t w0, int64_t nw, DevState &G, SceneDev &gsc)
{
    G = S;
    gsc = sc;
    const int64_t g0 = w0 * S.N;
    G.W = (int32_t)nw;
    G.A = nw * S.N;
    gsc.worldOffset = sc.worldOffset + (uint32_t)w0;
#define MP_SL_A(n) G.n = S.n + g0;
#define MP_SL_W(n) G.n = S.n + w0;
    MP_AGENT_F32(MP_SL_A)
    MP_AGENT_I32(MP_SL_A)
    MP_WORLD_I32(MP_SL_W)
    MP_WORLD_F32(MP_SL_W)
#undef MP_SL_A
#undef MP_SL_W
    const int64_t T = S.T, trackLen = sc.spawnTrackLen; // the buffer table's run-time row shapes
#define MP_SL(n, type, kind, ...) G.n = S.n + bufFirstRow(kind, w0, S.N) * rowElems(__VA_ARGS__);
#define MP_SL_E(n, type, kind, id, ...) MP_SL(n, type, kind, __VA_ARGS__)
    MP_BUFS(MP_SL, MP_SL_E)
#undef MP_SL
#undef MP_SL_E
    G.outBase = S.outBase + g0;
    G.dmg = S.dmg + g0; // stride stays S.dmgStride
    G.resetKeys = S.resetKeys + g0 * 11;
    if (S.recordLog) G.recordLog = S.recordLog + w0;
    if (S.replayLog) G.replayLog = S.replayLog + w0;
    if (S.events) G.events = S.events + w0 * S.evStride;
    if (S.snapshots) G.snapshots = S.snapshots + w0;
}

void mpenv_manager::setupGroups(int want)
{
    // the new split is built aside and swapped in whole: a throw leaves the
    // previous one in place; the previous one goes with the locals
    // at most 3 (4 measured slower: 66 vs 86 M agent-steps/s at C3)
    const MapRange &all = ranges[0];
    const int n = std::max(1, std::min(std::min(want, 3), all.n));
    Event fork;
    std::vector<SideStream> side;
    std::vector<MapRange> cut;
    if (n > 1) fork = Event::create(hipEventDisableTiming);
    for (int i = 0; i < n && n > 1; i++) {
        const int64_t w0 = (int64_t)all.n * i / n, w1 = (int64_t)all.n * (i + 1) / n;
        MapRange g;
        g.scene = all.scene;
        g.w0 = all.w0 + (int32_t)w0;
        g.n = (int32_t)(w1 - w0);
        sliceState(all.S, all.sc, w0, w1 - w0, g.S, g.sc);
        cut.push_back(g);
        if (i > 0) side.push_back(SideStream::create());
    }
    groups = n;
    std::swap(forkEv, fork);
    gside.swap(side);
    groupRanges.swap(cut);
}

// Workload counters on (the buffer) or off (null): in the batch and in every
// slice a kernel launches with.
void mpenv_manager::setStats(unsigned long long *p)
{
    S.stats = p;
    for (MapRange &r : ranges) r.S.stats = p;
    for (MapRange &g : groupRanges) g.S.stats = p;
}

// Live managers: the XLA targets receive a manager pointer inside opaque
// bytes XLA keeps, so they check it against this set before using it (a
// dropped SimManager, or foreign bytes, is then an error, not a read of freed
// memory).
static std::mutex g_liveMu;
static std::unordered_set<const mpenv_manager *> g_live;

static void liveAdd(const mpenv_manager *m)
{
    std::lock_guard<std::mutex> lk(g_liveMu);
    g_live.insert(m);
}

static void liveRemove(const mpenv_manager *m)
{
    std::lock_guard<std::mutex> lk(g_liveMu);
    g_live.erase(m);
}

static bool liveHas(const mpenv_manager *m)
{
    std::lock_guard<std::mutex> lk(g_liveMu);
    return g_live.count(m) != 0;
}

extern "C" {

int32_t mpenv_abi_version(void) { return MPENV_ABI_VERSION; }

const char *mpenv_last_error(void) { return g_last_error.c_str(); }

// mpenv_create (plan null: cfg->scene_path as one scene and one range over
// the batch) and mpenv_create_maps (the planned list, cfg->scene_path null).
static int createManager(const mpenv_config *cfg, MapPlan *plan, mpenv_manager **out)
{
    if (cfg->exec_mode != MPENV_EXEC_CUDA)
        return fail(MPENV_ERR_UNSUPPORTED, "ExecMode.CPU is not supported: this engine runs only on the GPU (HIP)");
    if (cfg->task_type != MPENV_TASK_ZONE && cfg->task_type != MPENV_TASK_ZONE_CAPTURE_DEFEND)
        return fail(MPENV_ERR_UNSUPPORTED, "only Task.Zone and Task.ZoneCaptureDefend are implemented");
    if (cfg->team_size < 1 || cfg->team_size > kMaxTeamSize)
        return fail(MPENV_ERR_INVALID, "team_size must be in [1, 6]");
    if (cfg->num_worlds == 0) return fail(MPENV_ERR_INVALID, "num_worlds must be > 0");
    if (!plan && !cfg->scene_path) return fail(MPENV_ERR_INVALID, "scene_path is required");
    if (cfg->sim_flags >> 12) return fail(MPENV_ERR_INVALID, "sim_flags has bits beyond SubZones (1 << 11)");
    if (cfg->replay_log_path && cfg->record_log_path)
        return fail(MPENV_ERR_UNSUPPORTED, "record and replay logs together are not supported");

    return guarded([&]() -> int {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
            return fail(MPENV_ERR_HIP, "no HIP device available");
        if (cfg->gpu_id < 0 || cfg->gpu_id >= ndev) return fail(MPENV_ERR_INVALID, "gpu_id out of range");
        HIP_CHECK(hipSetDevice(cfg->gpu_id));
        std::unique_ptr<mpenv_manager> m(new mpenv_manager()); // a throw below deletes it
        m->S.stats = nullptr;
        m->S.obsGate = nullptr;
        m->S.outTab = nullptr;
        m->S.outBase = 0;
        m->cfg = *cfg;
        m->gpu = cfg->gpu_id;
        m->fromList = plan != nullptr;
        // A blocking stream: ordered after work the caller queued on the
        // legacy default stream (e.g. torch writes into the action tensors),
        // matching the synchronous Manager::step contract (mgr.cpp:1949-1960).
        m->stream = Stream::create(hipStreamDefault);
        MapPlan one; // mpenv_create: the one scene, the one range over the batch
        if (!plan) {
            MapScene ms;
            ms.path = cfg->scene_path;
            ms.scene = loadScene(ms.path, (cfg->sim_flags & MPENV_SIMFLAG_SPAWN_IN_MIDDLE) != 0);
            ms.limits = sceneLimits(ms.scene);
            if (!ms.limits.supported) return fail(MPENV_ERR_UNSUPPORTED, "scene not supported: " + ms.limits.reason);
            one.scenes.push_back(std::move(ms));
            MapRange all;
            all.n = (int32_t)cfg->num_worlds;
            one.ranges.push_back(all);
            plan = &one;
        }
        m->scenes = std::move(plan->scenes);
        m->ranges = std::move(plan->ranges); // scene, w0, n; cut below
        m->cfg.scene_path = m->firstScene().path.c_str(); // the string at its final address
        // the per-scene device work once per loaded scene; spawnTrackLen, a
        // row shape of the buffer table, is the plan's largest in every
        // SceneDev (a range whose own value is smaller leaves the rows'
        // tails at their reset fill)
        int32_t trackLen = 0;
        for (MapScene &ms : m->scenes) {
            buildSceneDev(*m, ms.scene, ms.limits, ms.sc, ms.img);
            trackLen = std::max(trackLen, ms.sc.spawnTrackLen);
        }
        for (MapScene &ms : m->scenes) ms.sc.spawnTrackLen = trackLen;
        m->S.W = (int32_t)cfg->num_worlds;
        m->S.T = (int32_t)cfg->team_size;
        m->S.N = 2 * m->S.T;
        m->S.A = (int64_t)m->S.W * m->S.N;
        m->S.nMagic = (uint32_t)((0x100000000ull + (uint64_t)m->S.N - 1) / (uint64_t)m->S.N);
        if ((uint64_t)m->S.A * (uint64_t)m->S.N * (uint64_t)m->S.N >= 0x100000000ull)
            throw std::runtime_error("mpenv: num_worlds too large for one device (agent index division)");
        allocState(*m);
        openLogs(*m, cfg);
        m->stateRefused = cfg->replay_log_path  ? "a manager opened with replay_log_path"
                          : cfg->record_log_path ? "a manager opened with record_log_path"
                          : cfg->event_log_path  ? "a manager opened with event_log_path"
                                                 : nullptr;
        m->stateTabDev = m->alloc<StateTab>(1);
        buildStateTab(m->S, m->firstScene().sc, m->stateTabDev, m->stateTab);
        // the ranges as complete engines
        for (MapRange &r : m->ranges) sliceState(m->S, m->scenes[r.scene].sc, r.w0, r.n, r.S, r.sc);
        if (m->mapSet()) {
            // from a list: the world -> range table, and the checkpoint
            // header's hash of the layout (reserved[0..1]; zeros for a manager
            // from mpenv_create, whose table mpenv_map_of_world makes): FNV-1a
            // 64 over each range's world count and its scene's collisions.bin hash
            std::vector<int32_t> mow((size_t)m->S.W);
            uint64_t h = 1469598103934665603ull;
            auto mix = [&h](uint64_t v) {
                for (int b = 0; b < 8; b++) {
                    h ^= (v >> (8 * b)) & 0xffu;
                    h *= 1099511628211ull;
                }
            };
            for (size_t k = 0; k < m->ranges.size(); k++) {
                const MapRange &r = m->ranges[k];
                std::fill(mow.begin() + r.w0, mow.begin() + r.w0 + r.n, (int32_t)k);
                m->stateTab.rangeScene[k] = r.scene;
                mix((uint64_t)r.n);
                mix(m->scenes[r.scene].collisionsHash);
            }
            m->mapOfWorld = m->alloc<int32_t>(mow.size());
            m->upload(m->mapOfWorld, mow.data(), mow.size() * sizeof(int32_t));
            m->stateTab.mapOfWorld = m->mapOfWorld;
            m->stateTab.hdr.reserved[0] = (uint32_t)h;
            m->stateTab.hdr.reserved[1] = (uint32_t)(h >> 32);
        }
        m->upload(m->stateTabDev, &m->stateTab, sizeof(StateTab));
        // the caller's path strings are not kept past create
        m->cfg.replay_log_path = m->cfg.record_log_path = m->cfg.event_log_path = nullptr;
        m->cfg.curriculum_data_path = nullptr;
        {
            // World groups (concurrent streams).  MPENV_WORLD_GROUPS overrides.
            // Two measured best at C3 in rounds 2-4 (round 2: 1.447 ms/step
            // against 1.468 with one); since round 5's load-first k_obs one
            // group is faster (driver window 1.23 vs 1.30 ms, steady 1.178 vs
            // 1.215; profiles/r05e_ab_world_groups.jsonl).
            int want = 1;
            if (const char *e = std::getenv("MPENV_WORLD_GROUPS")) want = std::atoi(e);
            m->setupGroups(m->mapSet() ? 1 : want); // a map set's ranges are its groups
        }
        if (const char *e = std::getenv("MPENV_SCENE_RESIDENCY")) {
            const std::string v = e;
            const int32_t mode = v == "auto" ? MPENV_SCENE_AUTO : v == "lds" ? MPENV_SCENE_LDS
                                 : v == "global"                             ? MPENV_SCENE_GLOBAL
                                                                             : -1;
            if (mpenv_set_scene_residency(m.get(), mode) != MPENV_OK)
                throw std::runtime_error("MPENV_SCENE_RESIDENCY=" + v + ": " + g_last_error);
        }
        if (const char *e = std::getenv("MPENV_STEP_GRAPH")) m->useGraph = std::atoi(e) != 0;
        if (const char *e = m->mapSet() ? nullptr : std::getenv("MPENV_LIDAR_BRANCH"))
            if (std::atoi(e) != 0 && mpenv_set_lidar_branch(m.get(), 1) != MPENV_OK) throw std::runtime_error(g_last_error);
        // TrainControl from sim flags (mgr.cpp:1397-1413)
        int32_t tc[3] = { (cfg->sim_flags & MPENV_SIMFLAG_SIM_EVAL_MODE) ? 1 : 0,
                          (cfg->sim_flags & MPENV_SIMFLAG_STAGGER_STARTS) ? 1 : 0,
                          (cfg->sim_flags & MPENV_SIMFLAG_RANDOM_FLIP_TEAMS) ? 1 : 0 };
        HIP_CHECK(hipMemcpyAsync(m->S.trainCtrl, tc, sizeof(tc), hipMemcpyHostToDevice, m->stream));
        for (const MapRange &r : m->ranges) launched(launchConstruct(r.S, r.sc, tc, m->stream), "construct launch failed");
        HIP_CHECK(hipStreamSynchronize(m->stream));
        liveAdd(m.get());
        *out = m.release();
        return MPENV_OK;
    });
}

int mpenv_create(const mpenv_config *cfg, mpenv_manager **out)
{
    if (!cfg || !out) return fail(MPENV_ERR_INVALID, "null argument");
    *out = nullptr;
    return createManager(cfg, nullptr, out);
}

// Map sets (mpenv_maps.h; DESIGN.md §2 definition 19)
int mpenv_create_maps(const mpenv_config *cfg, const mpenv_map_range *maps, int32_t n, mpenv_manager **out)
{
    if (!cfg || !maps || !out) return fail(MPENV_ERR_INVALID, "null argument");
    *out = nullptr;
    for (const char *p : { cfg->replay_log_path, cfg->record_log_path, cfg->event_log_path, cfg->curriculum_data_path })
        if (p)
            return fail(MPENV_ERR_UNSUPPORTED, "map set: replay_log_path, record_log_path, event_log_path and "
                                               "curriculum_data_path are not supported (logged and snapshot "
                                               "positions belong to one map)");
    MapPlan plan;
    const int rc = guarded([&]() -> int { return planMaps(*cfg, maps, n, plan, nullptr); }, MPENV_ERR_INVALID);
    if (rc != MPENV_OK) return rc;
    return createManager(cfg, &plan, out);
}

static int mapSetRefused(const mpenv_manager *m, const char *what, const char *why)
{
    if (!m->mapSet()) return MPENV_OK;
    return fail(MPENV_ERR_UNSUPPORTED, std::string(what) + " is not supported on a map-set manager: " + why);
}

int mpenv_num_maps(mpenv_manager *m, int32_t *n)
{
    if (!m || !n) return fail(MPENV_ERR_INVALID, "null argument");
    *n = (int32_t)m->ranges.size();
    return MPENV_OK;
}

int mpenv_map_info(mpenv_manager *m, int32_t range, mpenv_map_desc *out, const char **scene_path)
{
    if (!m || !out) return fail(MPENV_ERR_INVALID, "null argument");
    const int32_t n = (int32_t)m->ranges.size();
    if (range < 0 || range >= n)
        return fail(MPENV_ERR_INVALID, "map range " + std::to_string(range) + " is outside [0, " + std::to_string(n) + ")");
    std::memset(out, 0, sizeof(*out));
    out->supported = 1;
    const MapRange &r = m->ranges[(size_t)range];
    const MapScene &ms = m->scenes[r.scene];
    out->first_world = r.w0;
    out->num_worlds = r.n;
    out->scene = r.scene;
    if (scene_path) *scene_path = ms.path.c_str();
    out->residency = ms.img.residency == kResidencyLds ? MPENV_SCENE_LDS : MPENV_SCENE_GLOBAL;
    return MPENV_OK;
}

int mpenv_map_of_world(mpenv_manager *m, void **dev_ptr)
{
    if (!m || !dev_ptr) return fail(MPENV_ERR_INVALID, "null argument");
    return guarded([&] {
        // a manager from mpenv_create: all zeros, made on first use
        if (!m->mapOfWorld) {
            m->mapOfWorld = m->alloc<int32_t>((size_t)m->S.W);
            HIP_CHECK(hipStreamSynchronize(m->stream));
        }
        *dev_ptr = m->mapOfWorld;
    });
}

void mpenv_destroy(mpenv_manager *m)
{
    if (m) liveRemove(m);
    delete m;
}

int mpenv_init(mpenv_manager *m)
{
    if (!m) return fail(MPENV_ERR_INVALID, "null manager");
    return guarded([&] {
        m->runInitGraph(m->stream);
        m->exportsStale = false;
        HIP_CHECK(hipStreamSynchronize(m->stream));
    });
}

int mpenv_step_async(mpenv_manager *m, void *stream)
{
    if (!m) return fail(MPENV_ERR_INVALID, "null manager");
    return guarded([&] {
        m->runStep(streamOf(m, stream));
        m->exportsStale = false;
    });
}

int mpenv_step(mpenv_manager *m)
{
    if (!m) return fail(MPENV_ERR_INVALID, "null manager");
    return guarded([&] {
        m->runStep(m->stream);
        m->exportsStale = false;
        HIP_CHECK(hipStreamSynchronize(m->stream));
    });
}

int mpenv_export_tensor(mpenv_manager *m, int32_t id, void **ptr, int32_t *dtype, int32_t *ndim, int64_t *dims,
                        int32_t *gpu_id)
{
    if (!m || !ptr || !dtype || !ndim || !dims) return fail(MPENV_ERR_INVALID, "null argument");
    return guarded([&] {
        TensorDesc d;
        if (!m->exportDesc(id, d)) return fail(MPENV_ERR_INVALID, "unknown export id " + std::to_string(id));
        *ptr = d.ptr;
        *dtype = d.dtype;
        *ndim = (int32_t)d.dims.size();
        for (size_t k = 0; k < d.dims.size(); k++) dims[k] = d.dims[k];
        if (gpu_id) *gpu_id = m->gpu;
        return MPENV_OK;
    });
}

int mpenv_export_layout(int32_t id, uint32_t num_worlds, uint32_t team_size, int32_t *dtype, int32_t *ndim,
                        int64_t *dims)
{
    if (!dtype || !ndim || !dims) return fail(MPENV_ERR_INVALID, "null argument");
    if (num_worlds == 0 || team_size == 0 || team_size > (uint32_t)kMaxTeamSize)
        return fail(MPENV_ERR_INVALID, "num_worlds must be >= 1 and team_size in [1, 6]");
    TensorDesc d;
    if (!exportLayout(id, num_worlds, 2 * (int64_t)team_size, d))
        return fail(MPENV_ERR_INVALID, "unknown export id " + std::to_string(id));
    *dtype = d.dtype;
    *ndim = (int32_t)d.dims.size();
    for (size_t k = 0; k < d.dims.size(); k++) dims[k] = d.dims[k];
    return MPENV_OK;
}

int mpenv_train_interface_size(int32_t *num_inputs, int32_t *num_outputs)
{
    if (num_inputs) *num_inputs = kNumTIInputs;
    if (num_outputs) *num_outputs = kNumTIOutputs;
    return MPENV_OK;
}

int mpenv_train_interface_entry(int32_t is_output, int32_t idx, const char **name, int32_t *export_id)
{
    const TIEntry *tab = is_output ? kTIOutputs : kTIInputs;
    int n = is_output ? kNumTIOutputs : kNumTIInputs;
    if (idx < 0 || idx >= n) return fail(MPENV_ERR_INVALID, "train interface index out of range");
    if (name) *name = tab[idx].name;
    if (export_id) *export_id = tab[idx].id;
    return MPENV_OK;
}

// The refusal of a call that reads the engine's own observation rows
// (masks, filters, self, teammate and opponent rows, the three position
// rows) while the last step was a direct mpenv_gpu_stream_step, which wrote
// them into its caller's buffers only: MPENV_OK when they are current.
static int staleExports(const mpenv_manager *m, const char *who, const char *instead)
{
    if (!m->exportsStale) return MPENV_OK;
    return fail(MPENV_ERR_INVALID, std::string(who) + ": the last mpenv_gpu_stream_step wrote the observations into "
                                       "its caller's buffers only; " + instead);
}

// cudaCopyStepInputs / cudaCopyStepOutputs (mgr.cpp:614-645): every
// trainInterface input from the caller's buffers, or every output into
// them, as one batched copy launch (the agent maps are never written by the
// step and stay all zeros, so their copies are zero fills); a segment whose
// pointers are not 16-B aligned falls back to hipMemcpyAsync.
// `what` selects the segments.
enum TISel : unsigned {
    kSelInputs = 1, // every input, caller -> engine
    kSelState = 2,  // the outputs that are only ever copied (hp, rewards, last-known rows, ...)
    kSelDirect = 4, // the outputs an OutTab can take instead (TIEntry::direct)
    kSelZeros = 8,  // the agent maps' zero fills
};

// The call's OutTab: every output with TIEntry::direct set written straight
// into the caller's buffer; or false when one of those buffers is missing or
// not 16-B aligned (the kernels store float4 rows): then every output is
// copied as before.
static bool directTable(void **buffers, OutTab &t)
{
    t = OutTab {};
    t.on = 1;
    for (int i = 0; i < kNumTIOutputs; i++) {
        if (!kTIOutputs[i].direct) continue;
        float *p = static_cast<float *>(buffers[kNumTIInputs + i]);
        if (!p || ((uintptr_t)p & 15u)) return false;
        t.*kTIOutputs[i].direct = p;
    }
    return true;
}

static int copyTI(mpenv_manager *m, hipStream_t st, void **buffers, unsigned what, const OutTab *tab = nullptr)
{
    CopyBatch b {};
    if (tab) { // the out table rides the first copy launch (engine.h CopyBatch)
        b.tabDst = m->outTabDev;
        b.tab = *tab;
    }
    auto add = [&](const void *src, void *dst, size_t bytes) {
        if (((uintptr_t)src | (uintptr_t)dst) & 15u) {
            if (src) HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
            else HIP_CHECK(hipMemsetAsync(dst, 0, bytes, st));
            return;
        }
        if (b.n == kMaxCopySegs) {
            launched(launchCopyBatch(b, st), "copy launch failed");
            b.n = 0;
            b.tabDst = nullptr;
        }
        b.seg[b.n++] = CopySeg { src, dst, (int64_t)bytes };
    };
    int k = 0;
    for (int i = 0; i < kNumTIInputs; i++, k++) {
        if (!(what & kSelInputs) || !buffers[k]) continue;
        TensorDesc d;
        m->exportDesc(kTIInputs[i].id, d);
        add(buffers[k], d.ptr, d.bytes());
    }
    for (int i = 0; i < kNumTIOutputs; i++, k++) {
        const TIEntry &e = kTIOutputs[i];
        if (!(what & (e.zero ? kSelZeros : e.direct ? kSelDirect : kSelState)) || !buffers[k]) continue;
        TensorDesc d;
        m->exportDesc(e.id, d);
        add(e.zero ? nullptr : d.ptr, buffers[k], d.bytes());
    }
    if (b.n > 0 || b.tabDst) launched(launchCopyBatch(b, st), "copy launch failed");
    return 0;
}

// A side stream and the fork event that starts it, made on first use: both
// or, on a throw, neither.  gpuStreamStep's for the zero fills is made by
// gpuStreamInit (outside any graph capture of the steps that follow).
static void ensureSide(SideStream &side, Event &fork)
{
    if (side) return;
    SideStream s = SideStream::create();
    fork = Event::create(hipEventDisableTiming);
    side = std::move(s);
}

// mgr.cpp:507-612
int mpenv_gpu_stream_init(mpenv_manager *m, void *stream, void **buffers)
{
    if (!m || !buffers) return fail(MPENV_ERR_INVALID, "null argument");
    return guarded([&] {
        ensureSide(m->zSide, m->zForkEv);
        hipStream_t st = streamOf(m, stream);
        m->runInitGraph(st);
        m->exportsStale = false;
        copyTI(m, st, buffers, kSelState | kSelDirect | kSelZeros);
    });
}

// mgr.cpp:614-645
int mpenv_gpu_stream_step(mpenv_manager *m, void *stream, void **buffers)
{
    if (!m || !buffers) return fail(MPENV_ERR_INVALID, "null argument");
    return guarded([&] {
        hipStream_t st = streamOf(m, stream);
        ensureSide(m->zSide, m->zForkEv);
        // The observation rows, the lidar and the agent maps' zeros go
        // straight into the caller's buffers (OutTab, set in front of the
        // step and cleared behind it, so the captured step graph is the same
        // for every call); the rest -- the state-backed outputs (hp,
        // magazine, alive, last-known rows, rewards, dones, episode results)
        // -- is copied after the step.
        // with a policy loaded the step writes the engine's own observation
        // rows (the network's inputs at the next step) and every output is copied
        OutTab tab;
        const bool direct = !m->polLoaded && directTable(buffers, tab);
        m->exportsStale = direct;
        if (!direct) {
            // every output copied: the zero fills (1.6 GB of stores at C3)
            // beside the step, ordered after whatever the caller queued
            HIP_CHECK(hipEventRecord(m->zForkEv, st));
            m->zSide.startAfter(m->zForkEv);
            copyTI(m, m->zSide.stream, buffers, kSelZeros);
            m->zSide.markDone();
        }
        const OutTab off {};
        copyTI(m, st, buffers, kSelInputs, direct ? &tab : nullptr); // sets the table
        m->runStep(st);
        copyTI(m, st, buffers, direct ? kSelState : kSelState | kSelDirect, direct ? &off : nullptr); // clears it
        if (!direct) m->zSide.joinInto(st);
    });
}

int mpenv_debug_trace_rays(mpenv_manager *m, const float *o, const float *d, int32_t n, int32_t mode, float *t_out,
                           int32_t *hit_out, void *stream)
{
    if (!m || !o || !d || !t_out || !hit_out || n < 0) return fail(MPENV_ERR_INVALID, "bad argument");
    hipStream_t st = streamOf(m, stream);
    const MapScene &ms = m->firstScene();
    if (launchTraceRays(ms.sc, ms.img, o, d, n, mode, t_out, hit_out, st) || hipStreamSynchronize(st) != hipSuccess)
        return fail(MPENV_ERR_HIP, "trace-ray launch failed");
    return MPENV_OK;
}

int mpenv_debug_geom_queries(mpenv_manager *m, int32_t mode, int32_t n, const mpenv_geom_queries *q, void *stream)
{
    if (!m || !q || n < 0) return fail(MPENV_ERR_INVALID, "bad argument");
    const bool caps = mode == MPENV_GEOM_WORLD_RAY || mode == MPENV_GEOM_SIGHT;
    const bool casts = mode == MPENV_GEOM_CASTS;
    bool ok = mode >= MPENV_GEOM_LIDAR_RAY && mode <= MPENV_GEOM_STUCK && q->o && q->d;
    ok = ok && (mode == MPENV_GEOM_SIGHT || q->t) && (mode == MPENV_GEOM_CASTS || mode == MPENV_GEOM_STUCK || q->i0);
    if (caps) ok = ok && q->caps && q->sel && q->num_caps >= 1 && q->num_caps <= 12;
    if (mode == MPENV_GEOM_WORLD_RAY) ok = ok && q->i1;
    if (mode == MPENV_GEOM_SIGHT) ok = ok && (q->sub == 1 || (q->sub == 0 && q->hint));
    if (casts) ok = ok && q->sub >= 0 && q->sub <= 3 && (q->sub == 3 || q->normal) && (q->sub == 0 || q->bound) &&
                     (q->sub != 2 || (q->z1 && q->sel));
    if (mode == MPENV_GEOM_STUCK) ok = ok && q->sel && q->bound && n % 64 == 0;
    if (!ok) return fail(MPENV_ERR_INVALID, "bad geometry query");
    hipStream_t st = streamOf(m, stream);
    const MapScene &ms = m->firstScene();
    if (launchGeomQueries(ms.sc, ms.img, mode, n, *q, st) || hipStreamSynchronize(st) != hipSuccess)
        return fail(MPENV_ERR_HIP, "geometry-query launch failed");
    return MPENV_OK;
}

// XLA GPU custom-call targets (SimManager.jax(); include/mpenv.h)
static std::atomic<int64_t> g_xlaErrors { 0 };

int mpenv_xla_opaque_make(mpenv_manager *m, mpenv_xla_opaque *out)
{
    if (!m || !out) return fail(MPENV_ERR_INVALID, "null argument");
    *out = mpenv_xla_opaque {};
    out->magic = MPENV_XLA_MAGIC;
    out->version = MPENV_XLA_VERSION;
    out->manager = (uint64_t)(uintptr_t)m;
    out->num_buffers = kNumTIInputs + kNumTIOutputs;
    return MPENV_OK;
}

// The manager an opaque names, or null (with mpenv_last_error set) when the
// bytes are not an opaque of this build or name no live manager.
static mpenv_manager *xlaManager(const char *opaque, size_t len)
{
    mpenv_xla_opaque o;
    if (!opaque || len != sizeof(o)) {
        fail(MPENV_ERR_INVALID, "bad XLA opaque: " + std::to_string(len) + " bytes, expected " +
                                    std::to_string(sizeof(o)));
        return nullptr;
    }
    std::memcpy(&o, opaque, sizeof(o));
    if (o.magic != MPENV_XLA_MAGIC || o.version != MPENV_XLA_VERSION || o.num_buffers != kNumTIInputs + kNumTIOutputs) {
        fail(MPENV_ERR_INVALID, "bad XLA opaque: not made by mpenv_xla_opaque_make of this build");
        return nullptr;
    }
    mpenv_manager *m = reinterpret_cast<mpenv_manager *>((uintptr_t)o.manager);
    if (!liveHas(m)) {
        fail(MPENV_ERR_INVALID, "bad XLA opaque: its manager was destroyed (keep the SimManager alive while the "
                                "registered custom call is in use)");
        return nullptr;
    }
    return m;
}

static int xlaRun(bool step, void *stream, void **buffers, const char *opaque, size_t opaque_len)
{
    mpenv_manager *m = xlaManager(opaque, opaque_len);
    if (!m) return MPENV_ERR_INVALID;
    return step ? mpenv_gpu_stream_step(m, stream, buffers) : mpenv_gpu_stream_init(m, stream, buffers);
}

// API version 1 has no error channel: like the reference's REQ_CUDA / FATAL
// (mgr.cpp:514-531, 620-638) a failure is reported on stderr and aborts the
// process rather than leaving XLA with result buffers that were never written.
[[noreturn]] static void xlaFatal(const char *what)
{
    std::fprintf(stderr, "mpenv: XLA custom call %s failed: %s\n", what, g_last_error.c_str());
    std::fflush(stderr);
    std::abort();
}

void mpenv_xla_gpu_stream_init(void *stream, void **buffers, const char *opaque, size_t opaque_len)
{
    if (xlaRun(false, stream, buffers, opaque, opaque_len) != MPENV_OK) xlaFatal("gpuStreamInit");
}

void mpenv_xla_gpu_stream_step(void *stream, void **buffers, const char *opaque, size_t opaque_len)
{
    if (xlaRun(true, stream, buffers, opaque, opaque_len) != MPENV_OK) xlaFatal("gpuStreamStep");
}

// API_VERSION_STATUS_RETURNING: the failure goes to XLA through
// XlaCustomCallStatusSetFailure, exported by the XLA runtime that calls the
// target (jaxlib); it is looked up at run time so this library links without
// XLA.  Without it there is no one to hand the status to: abort as above.
typedef void (*XlaStatusSetFailureFn)(void *status, const char *message, size_t message_len);

static void xlaStatusFail(const char *what, void *status)
{
    static XlaStatusSetFailureFn fn =
        reinterpret_cast<XlaStatusSetFailureFn>(dlsym(RTLD_DEFAULT, "XlaCustomCallStatusSetFailure"));
    if (!fn || !status) xlaFatal(what);
    g_xlaErrors.fetch_add(1);
    const std::string msg = std::string("mpenv: ") + what + ": " + g_last_error;
    fn(status, msg.data(), msg.size());
}

void mpenv_xla_gpu_stream_init_status(void *stream, void **buffers, const char *opaque, size_t opaque_len,
                                      void *status)
{
    if (xlaRun(false, stream, buffers, opaque, opaque_len) != MPENV_OK) xlaStatusFail("gpuStreamInit", status);
}

void mpenv_xla_gpu_stream_step_status(void *stream, void **buffers, const char *opaque, size_t opaque_len,
                                      void *status)
{
    if (xlaRun(true, stream, buffers, opaque, opaque_len) != MPENV_OK) xlaStatusFail("gpuStreamStep", status);
}

int64_t mpenv_xla_errors(void) { return g_xlaErrors.load(); }

// Learner exchange wire format (wire.hip)
static const char *const kWireWhy = "the message is one view over the batch and its observation kernel takes one scene "
                                    "(the gather and local exchanges work)";
int mpenv_wire_bytes(mpenv_manager *m, int32_t keyframe, int64_t *bytes)
{
    if (!m || !bytes) return fail(MPENV_ERR_INVALID, "null argument");
    if (int rc = mapSetRefused(m, "mpenv_wire_bytes", kWireWhy)) return rc;
    *bytes = wireBytes(m->S, keyframe != 0);
    return MPENV_OK;
}

int mpenv_wire_pack(mpenv_manager *m, void *dst, int32_t keyframe, void *stream)
{
    if (!m || !dst) return fail(MPENV_ERR_INVALID, "null argument");
    if (int rc = mapSetRefused(m, "mpenv_wire_pack", kWireWhy)) return rc;
    if ((uintptr_t)dst & 15u) return fail(MPENV_ERR_INVALID, "wire message buffer must be 16-B aligned");
    if (launchWirePack(m->S, static_cast<char *>(dst), keyframe != 0, m->firstScene().sc.worldOffset, streamOf(m, stream)))
        return fail(MPENV_ERR_HIP, "wire pack launch failed");
    return MPENV_OK;
}

int mpenv_wire_unpack(mpenv_manager *m, const void *src, int32_t keyframe, void *stream)
{
    if (!m || !src) return fail(MPENV_ERR_INVALID, "null argument");
    if (int rc = mapSetRefused(m, "mpenv_wire_unpack", kWireWhy)) return rc;
    if ((uintptr_t)src & 15u) return fail(MPENV_ERR_INVALID, "wire message buffer must be 16-B aligned");
    void *st = streamOf(m, stream);
    const int W = m->S.W;
    int32_t *prev = m->wireEp + (size_t)m->wireParity * W, *next = m->wireEp + (size_t)(m->wireParity ^ 1) * W;
    const SceneDev &sc = m->firstScene().sc;
    if (launchWireUnpack(m->S, sc, static_cast<const char *>(src), keyframe != 0, m->wireErr, sc.worldOffset, prev, next, st))
        return fail(MPENV_ERR_HIP, "wire unpack launch failed");
    m->wireParity ^= 1;
    return MPENV_OK;
}

// The error word's bits now; the refused bit is cleared by this read, the
// desync bit stays until a keyframe is unpacked (wire.hip wireOk).  `stream`
// null: the whole device is synchronised first (every unpack queued so far
// has run); otherwise the read is ordered on that stream only, and with a
// pinned `out` (hipHostMalloc / torch pin_memory) the call does not block:
// the value lands when the stream reaches it (record an event after the
// call and wait on it before reading *out).
int mpenv_wire_error_async(mpenv_manager *m, uint32_t *out, void *stream)
{
    if (!m || !out) return fail(MPENV_ERR_INVALID, "null argument");
    return guarded([&] {
        hipStream_t st = (hipStream_t)stream;
        HIP_CHECK(hipMemcpyAsync(out, m->wireErr, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        // clear REFUSED, keep DESYNC: one atomic AND on the device word
        launched(launchWireErrClear(m->wireErr, st), "wire error clear launch failed");
    });
}

int mpenv_wire_error(mpenv_manager *m, uint32_t *out)
{
    if (!m || !out) return fail(MPENV_ERR_INVALID, "null argument");
    return guarded([&] {
        HIP_CHECK(hipDeviceSynchronize());
        uint32_t v = 0;
        HIP_CHECK(hipMemcpy(&v, m->wireErr, sizeof(uint32_t), hipMemcpyDeviceToHost));
        *out = v;
        // the refused bit is cleared by this read; the desync bit stays until a
        // keyframe is unpacked (wire.hip wireOk)
        const uint32_t keep = v & MPENV_WIRE_ERR_DESYNC;
        HIP_CHECK(hipMemcpy(m->wireErr, &keep, sizeof(uint32_t), hipMemcpyHostToDevice));
    });
}

// World checkpoints (state.hip)
static int stateUsable(mpenv_manager *m, const void *buf, const char *what)
{
    if (!m || !buf) return fail(MPENV_ERR_INVALID, "null argument");
    if (m->stateRefused)
        return fail(MPENV_ERR_INVALID, std::string("state checkpoints are not available for ") + m->stateRefused +
                                           " (append-only log files would desynchronise)");
    if ((uintptr_t)buf & 15u) return fail(MPENV_ERR_INVALID, std::string(what) + " must be 16-B aligned");
    // a buffer inside one of the manager's allocations would alias live state
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)buf) == hipSuccess) {
        if (std::find(m->allocations.begin(), m->allocations.end(), (void *)base) != m->allocations.end())
            return fail(MPENV_ERR_INVALID, std::string(what) + " lies inside the manager's own allocations");
    } else {
        (void)hipGetLastError();
    }
    return MPENV_OK;
}

int mpenv_state_bytes(mpenv_manager *m, int64_t *bytes)
{
    if (!m || !bytes) return fail(MPENV_ERR_INVALID, "null argument");
    *bytes = m->stateTab.hdr.bytes;
    return MPENV_OK;
}

int mpenv_state_dims(mpenv_manager *m, uint32_t *num_worlds, uint32_t *team_size, uint32_t *spawn_track_len)
{
    if (!m) return fail(MPENV_ERR_INVALID, "null argument");
    if (num_worlds) *num_worlds = (uint32_t)m->S.W;
    if (team_size) *team_size = (uint32_t)m->S.T;
    if (spawn_track_len) *spawn_track_len = (uint32_t)m->firstScene().sc.spawnTrackLen;
    return MPENV_OK;
}

int mpenv_state_save(mpenv_manager *m, void *dst, void *stream)
{
    if (int rc = stateUsable(m, dst, "state snapshot buffer")) return rc;
    // the blob would hold observation rows from another step than its state
    if (int rc = staleExports(m, "mpenv_state_save", "save after a plain step")) return rc;
    if (launchStateSave(m->stateTab, m->stateTabDev, static_cast<char *>(dst), streamOf(m, stream)))
        return fail(MPENV_ERR_HIP, "state save launch failed");
    return MPENV_OK;
}

int mpenv_state_load(mpenv_manager *m, const void *src, const int32_t *map, void *stream)
{
    if (int rc = stateUsable(m, src, "state snapshot buffer")) return rc;
    if ((uintptr_t)map & 15u) return fail(MPENV_ERR_INVALID, "state world map must be 16-B aligned");
    // exportsStale stays as it is: the load is checked on the device and a
    // refused one (mpenv_state_error) writes nothing, so the host cannot know
    // that the observation rows are the blob's.  After a good load they are
    // current and mpenv_policy_load, mpenv_combat_actions and
    // mpenv_state_save are refused needlessly until the next plain step.
    if (launchStateLoad(m->stateTab, m->stateTabDev, static_cast<const char *>(src), map, streamOf(m, stream)))
        return fail(MPENV_ERR_HIP, "state load launch failed");
    return MPENV_OK;
}

int mpenv_state_error(mpenv_manager *m, uint32_t *bits)
{
    if (!m || !bits) return fail(MPENV_ERR_INVALID, "null argument");
    return guarded([&] {
        HIP_CHECK(hipDeviceSynchronize());
        uint32_t v = 0;
        HIP_CHECK(hipMemcpy(&v, &m->stateTabDev->err, sizeof(uint32_t), hipMemcpyDeviceToHost));
        *bits = v;
        if (v) HIP_CHECK(hipMemset(&m->stateTabDev->err, 0, sizeof(uint32_t)));
    });
}

int mpenv_state_section(int32_t idx, uint32_t num_worlds, uint32_t team_size, uint32_t spawn_track_len,
                        const char **name, int64_t *offset, int64_t *bytes, int32_t *row_bytes, int32_t *row_kind,
                        int32_t *export_id)
{
    if (num_worlds == 0 || team_size == 0 || team_size > (uint32_t)kMaxTeamSize)
        return fail(MPENV_ERR_INVALID, "num_worlds must be >= 1 and team_size in [1, 6]");
    if (spawn_track_len < (uint32_t)kMinSpawnTrack)
        return fail(MPENV_ERR_INVALID, "spawn_track_len must be >= " + std::to_string(kMinSpawnTrack));
    const int64_t W = num_worlds, N = 2 * (int64_t)team_size;
    StateSectionInfo si;
    if (idx == -1) {
        si = { "blob", 0, stateBytes(W, N, spawn_track_len), stateNumSections(), -1, -1, MPENV_DTYPE_UINT8, 0, -1 };
    } else if (!stateSection(idx, W, N, spawn_track_len, si)) {
        return fail(MPENV_ERR_INVALID, "state section index " + std::to_string(idx) + " out of range");
    }
    if (name) *name = si.name;
    if (offset) *offset = si.offset;
    if (bytes) *bytes = si.bytes;
    if (row_bytes) *row_bytes = si.rowBytes;
    if (row_kind) *row_kind = si.rowKind;
    if (export_id) *export_id = si.exportId;
    return MPENV_OK;
}

int mpenv_state_section_dtype(int32_t idx, int32_t *dtype)
{
    StateSectionInfo si;
    if (!dtype) return fail(MPENV_ERR_INVALID, "null argument");
    if (!stateSection(idx, 1, 2, kMinSpawnTrack, si))
        return fail(MPENV_ERR_INVALID, "state section index " + std::to_string(idx) + " out of range");
    *dtype = si.dtype;
    return MPENV_OK;
}

// In-sim policy inference (policy.cpp, policy.hip; DESIGN.md §2 definition 15)
int mpenv_policy_check(const char *dir)
{
    std::string err;
    const int rc = policyRead(dir, nullptr, err);
    return rc == MPENV_OK ? MPENV_OK : fail(rc, err);
}

static_assert(MPENV_POLICY_SLOTS == pol::kSlots, "mpenv_policy_slots.h and policy.h name the same slots");

static int policySlotRange(int32_t slot)
{
    if (slot >= 0 && slot < MPENV_POLICY_SLOTS) return MPENV_OK;
    return fail(MPENV_ERR_INVALID, "policy slot " + std::to_string(slot) + " is outside [0, " +
                                       std::to_string(MPENV_POLICY_SLOTS) + ")");
}

int mpenv_policy_load_slot(mpenv_manager *m, int32_t slot, const char *dir)
{
    if (!m || !dir) return fail(MPENV_ERR_INVALID, "null argument");
    if (int rc = policySlotRange(slot)) return rc;
    if (m->stateRefused)
        return fail(MPENV_ERR_INVALID, std::string("in-sim policy inference is not available for ") + m->stateRefused +
                                           " (the logged actions would not be the ones played)");
    if (m->cfg.sim_flags & MPENV_SIMFLAG_FULL_TEAM_POLICY)
        return fail(MPENV_ERR_INVALID, "in-sim policy inference is not available with SimFlags.FullTeamPolicy "
                                       "(the full-team action columns and the policy would write the same actions)");
    if (int rc = staleExports(m, "in-sim policy inference",
                              "load the policy before the first mpenv_gpu_stream_step or after a plain step"))
        return rc;
    std::vector<float> blob;
    std::string err;
    if (const int rc = policyRead(dir, &blob, err)) return fail(rc, err);
    // from here on only a HIP failure stops the load; the slot keeps its old
    // checkpoint until the new one is in device memory
    const int rc = guarded([&] {
        HIP_CHECK(hipSetDevice(m->gpu));
        HIP_CHECK(hipStreamSynchronize(m->stream));
        DevPtr fresh = DevPtr::create(blob.size() * sizeof(float));
        m->upload(fresh, blob.data(), blob.size() * sizeof(float));
        if (!m->polDev.blobs) m->allocPolicyWork();
        m->setPolicySlot(slot, static_cast<const float *>(fresh.get()));
        (void)fresh.release(); // the slot owns it now
    });
    if (rc != MPENV_OK && !m->polDev.mask) m->freePolicy();
    return rc;
}

int mpenv_policy_load(mpenv_manager *m, const char *dir) { return mpenv_policy_load_slot(m, 0, dir); }

int mpenv_policy_unload_slot(mpenv_manager *m, int32_t slot)
{
    if (!m) return fail(MPENV_ERR_INVALID, "null manager");
    if (int rc = policySlotRange(slot)) return rc;
    if (!m->polBlobs[slot]) return MPENV_OK;
    return guarded([&] {
        HIP_CHECK(hipSetDevice(m->gpu));
        HIP_CHECK(hipDeviceSynchronize()); // a step on a caller's stream may still read the blob
        m->setPolicySlot(slot, nullptr);
        if (!m->polDev.mask) m->freePolicy();
    });
}

int mpenv_policy_unload(mpenv_manager *m)
{
    if (!m) return fail(MPENV_ERR_INVALID, "null manager");
    (void)hipSetDevice(m->gpu);
    (void)hipDeviceSynchronize(); // a step on a caller's stream may still read the blobs
    m->freePolicy();
    return MPENV_OK;
}

int mpenv_policy_loaded(mpenv_manager *m, int32_t *on)
{
    if (!m || !on) return fail(MPENV_ERR_INVALID, "null argument");
    *on = m->polLoaded ? 1 : 0;
    return MPENV_OK;
}

int mpenv_policy_slots(mpenv_manager *m, uint32_t *mask)
{
    if (!m || !mask) return fail(MPENV_ERR_INVALID, "null argument");
    *mask = m->polDev.mask;
    return MPENV_OK;
}

int mpenv_policy_forward_slot(mpenv_manager *m, int32_t slot, float *logits, int32_t *actions, void *stream)
{
    if (!m || !logits) return fail(MPENV_ERR_INVALID, "null argument");
    if (int rc = policySlotRange(slot)) return rc;
    if (!m->polBlobs[slot])
        return fail(MPENV_ERR_INVALID, slot == 0 ? std::string("no policy loaded (mpenv_policy_load)")
                                                 : "policy slot " + std::to_string(slot) +
                                                       " is empty (mpenv_policy_load_slot)");
    if (launchPolicyForward(m->S, m->polDev, slot, logits, actions, streamOf(m, stream), m->polPrecision))
        return fail(MPENV_ERR_HIP, "policy launch failed");
    return MPENV_OK;
}

int mpenv_policy_forward(mpenv_manager *m, float *logits, int32_t *actions, void *stream)
{
    return mpenv_policy_forward_slot(m, 0, logits, actions, stream);
}

int mpenv_debug_policy_step(mpenv_manager *m, int32_t parts, void *stream)
{
    if (!m) return fail(MPENV_ERR_INVALID, "null manager");
    if (!m->polLoaded) return fail(MPENV_ERR_INVALID, "no policy loaded (mpenv_policy_load)");
    if (parts < 1 || parts > kPolicyAll) return fail(MPENV_ERR_INVALID, "policy step: parts must be in [1, 7]");
    if (launchPolicyStep(m->S, m->polDev, streamOf(m, stream), parts, m->polPrecision))
        return fail(MPENV_ERR_HIP, "policy launch failed");
    return MPENV_OK;
}

int mpenv_debug_policy_dense(mpenv_manager *m, const float *x, int32_t M, int32_t K, const float *w_host, int32_t N,
                             float *y, void *stream)
{
    if (!m || !x || !w_host || !y) return fail(MPENV_ERR_INVALID, "null argument");
    if (M < 1 || N < 1 || K < 1 || K > pol::kHidden)
        return fail(MPENV_ERR_INVALID, "policy dense: M, N >= 1 and 1 <= K <= 512");
    const int Np = (N + 63) / 64 * 64; // a wave takes two column tiles
    std::vector<float> wide((size_t)K * Np, 0.f), packed((size_t)pol::packedFloats(K, Np));
    for (int k = 0; k < K; k++) std::memcpy(&wide[(size_t)k * Np], &w_host[(size_t)k * N], sizeof(float) * (size_t)N);
    pol::packB(wide.data(), K, Np, packed.data());
    return guarded([&] {
        hipStream_t st = streamOf(m, stream);
        DevPtr wp = DevPtr::create(packed.size() * sizeof(float));
        HIP_CHECK(hipMemcpyAsync(wp, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice, st));
        launched(launchPolicyDense(x, M, K, static_cast<const float *>(wp.get()), N, y, st),
                 "policy dense launch failed");
        HIP_CHECK(hipStreamSynchronize(st));
    });
}

int mpenv_policy_set_precision(mpenv_manager *m, int32_t precision)
{
    if (!m) return fail(MPENV_ERR_INVALID, "null manager");
    if (precision != MPENV_POLICY_F32 && precision != MPENV_POLICY_BF16)
        return fail(MPENV_ERR_INVALID, "policy precision " + std::to_string(precision) +
                                           " is neither MPENV_POLICY_F32 (0) nor MPENV_POLICY_BF16 (1)");
    m->polPrecision = precision;
    return MPENV_OK;
}

int mpenv_policy_precision(mpenv_manager *m, int32_t *out)
{
    if (!m || !out) return fail(MPENV_ERR_INVALID, "null argument");
    *out = m->polPrecision;
    return MPENV_OK;
}

int mpenv_debug_policy_pack_bf16(const float *w, int32_t K, int32_t N, uint16_t *out, int64_t *count)
{
    if (!w || !count) return fail(MPENV_ERR_INVALID, "null argument");
    if (K < 1 || N < 1) return fail(MPENV_ERR_INVALID, "policy pack: K, N >= 1");
    *count = pol::packedBf16(K, N);
    if (out) pol::packBf16(w, K, N, out);
    return MPENV_OK;
}

int mpenv_debug_policy_dense_bf16(mpenv_manager *m, const float *x, int32_t M, int32_t K, const float *w_host,
                                  int32_t N, float *y, void *stream)
{
    if (!m || !x || !w_host || !y) return fail(MPENV_ERR_INVALID, "null argument");
    if (M < 1 || N < 1 || K < 1 || K > pol::kHidden)
        return fail(MPENV_ERR_INVALID, "policy dense: M, N >= 1 and 1 <= K <= 512");
    const int Np = (N + 63) / 64 * 64; // a wave takes two column tiles
    std::vector<float> wide((size_t)K * Np, 0.f);
    std::vector<uint16_t> packed((size_t)pol::packedBf16(K, Np));
    for (int k = 0; k < K; k++) std::memcpy(&wide[(size_t)k * Np], &w_host[(size_t)k * N], sizeof(float) * (size_t)N);
    pol::packBf16(wide.data(), K, Np, packed.data());
    return guarded([&] {
        hipStream_t st = streamOf(m, stream);
        DevPtr wp = DevPtr::create(packed.size() * sizeof(uint16_t));
        HIP_CHECK(hipMemcpyAsync(wp, packed.data(), packed.size() * sizeof(uint16_t), hipMemcpyHostToDevice, st));
        launched(launchPolicyDenseBf16(x, M, K, static_cast<const uint16_t *>(wp.get()), N, y, st),
                 "policy dense launch failed");
        HIP_CHECK(hipStreamSynchronize(st));
    });
}

int mpenv_graph_captures(mpenv_manager *m, int64_t *out)
{
    if (!m || !out) return fail(MPENV_ERR_INVALID, "null argument");
    *out = m->graphCaptures;
    return MPENV_OK;
}

int mpenv_graph_status(mpenv_manager *m, int32_t *graph_on, char *reason, int32_t reason_len)
{
    if (!m || !graph_on) return fail(MPENV_ERR_INVALID, "null argument");
    *graph_on = m->useGraph ? 1 : 0;
    if (reason && reason_len > 0) {
        std::snprintf(reason, (size_t)reason_len, "%s", m->graphOffReason.c_str());
    }
    return MPENV_OK;
}

int mpenv_set_lidar_branch(mpenv_manager *m, int32_t on)
{
    if (!m) return fail(MPENV_ERR_INVALID, "null argument");
    if (on)
        if (int rc = mapSetRefused(m, "mpenv_set_lidar_branch", "the ranges' kernels run in order on one stream")) return rc;
    return guarded([&] {
        HIP_CHECK(hipStreamSynchronize(m->stream));
        if (on) ensureSide(m->bSide, m->bForkEv);
        m->lidarBranch = on != 0;
    });
}

int mpenv_set_lidar_iters(mpenv_manager *m, int32_t n)
{
    if (!m) return fail(MPENV_ERR_INVALID, "null argument");
    if (n < 0 || n > lidarItersMax())
        return fail(MPENV_ERR_INVALID, "lidar iters must be 0 (automatic) or in [1, " + std::to_string(lidarItersMax()) + "]");
    // a kernel argument: the step graph is keyed on it (argKey) and re-captured
    m->lidarIters = n;
    return MPENV_OK;
}

int mpenv_set_world_groups(mpenv_manager *m, int32_t groups)
{
    if (!m || groups < 1) return fail(MPENV_ERR_INVALID, "bad argument");
    if (groups > 1)
        if (int rc = mapSetRefused(m, "mpenv_set_world_groups", "the ranges are the groups and run in order on one stream"))
            return rc;
    return guarded([&] {
        HIP_CHECK(hipStreamSynchronize(m->stream));
        m->setupGroups(groups);
    });
}

int mpenv_set_scene_residency(mpenv_manager *m, int32_t mode)
{
    if (!m) return fail(MPENV_ERR_INVALID, "null manager");
    if (mode != MPENV_SCENE_AUTO && mode != MPENV_SCENE_LDS && mode != MPENV_SCENE_GLOBAL)
        return fail(MPENV_ERR_INVALID, "scene residency must be MPENV_SCENE_AUTO, MPENV_SCENE_LDS or MPENV_SCENE_GLOBAL "
                                       "(MPENV_SCENE_RESIDENCY=auto|lds|global)");
    // every scene, or (one that does not fit; a list names it) none
    for (size_t r = 0; mode == MPENV_SCENE_LDS && r < m->ranges.size(); r++) {
        const MapScene &ms = m->scenes[m->ranges[r].scene];
        if (ms.limits.ldsOk) continue;
        const std::string which = m->mapSet() ? "map range " + std::to_string(r) + " (" + ms.path + ")" : "scene";
        return fail(MPENV_ERR_INVALID, which + " does not fit the LDS-resident path: " + ms.limits.ldsWhyNot);
    }
    return guarded([&] {
        // the kernels of a step in flight keep the path they were launched
        // on; the step graph is keyed on every img (argKey) and re-captured
        HIP_CHECK(hipStreamSynchronize(m->stream));
        m->residencyMode = mode;
        for (MapScene &ms : m->scenes) {
            const bool lds = mode == MPENV_SCENE_LDS || (mode == MPENV_SCENE_AUTO && ms.limits.ldsOk);
            ms.img.residency = lds ? kResidencyLds : kResidencyGlobal;
        }
    });
}

int mpenv_scene_residency(mpenv_manager *m, int32_t *mode_in_use)
{
    if (!m || !mode_in_use) return fail(MPENV_ERR_INVALID, "null argument");
    if (m->mapSet())
        return fail(MPENV_ERR_INVALID, "mpenv_scene_residency: a map set has a residency per map (mpenv_map_info)");
    *mode_in_use = m->firstScene().img.residency == kResidencyLds ? MPENV_SCENE_LDS : MPENV_SCENE_GLOBAL;
    return MPENV_OK;
}

int mpenv_world_groups(mpenv_manager *m, int32_t *groups)
{
    if (!m || !groups) return fail(MPENV_ERR_INVALID, "bad argument");
    *groups = m->groups;
    return MPENV_OK;
}

int mpenv_copy_actions(mpenv_manager *m, const int32_t *src, void *stream)
{
    if (!m || !src) return fail(MPENV_ERR_INVALID, "null argument");
    if (launchFillActions(m->S, src, streamOf(m, stream)))
        return fail(MPENV_ERR_HIP, "action copy launch failed");
    return MPENV_OK;
}

int mpenv_combat_actions(mpenv_manager *m, const int32_t *tape, int32_t *out, int32_t mode, void *stream)
{
    if (!m || !tape) return fail(MPENV_ERR_INVALID, "null argument");
    if (mode != 0 && mode != 1) return fail(MPENV_ERR_INVALID, "combat action mode must be 0 or 1");
    // the aim-bot would aim at the opponents of the last plain step
    if (int rc = staleExports(m, "mpenv_combat_actions", "call it after a plain step")) return rc;
    if (launchCombatActions(m->S, tape, out, mode, streamOf(m, stream)))
        return fail(MPENV_ERR_HIP, "combat action launch failed");
    return MPENV_OK;
}

static int checkAgent(mpenv_manager *m, int32_t w, int32_t a)
{
    if (!m) return fail(MPENV_ERR_INVALID, "null manager");
    if (w < 0 || w >= m->S.W) return fail(MPENV_ERR_INVALID, "world index out of range");
    if (a < 0 || a >= m->S.N) return fail(MPENV_ERR_INVALID, "agent index out of range");
    return MPENV_OK;
}

// Setter upload: ordered after in-flight work on the manager stream.
static bool put(mpenv_manager *m, void *dst, const void *src, size_t bytes)
{
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, m->stream) == hipSuccess &&
           hipStreamSynchronize(m->stream) == hipSuccess;
}

int mpenv_trigger_reset(mpenv_manager *m, int32_t w)
{
    if (int rc = checkAgent(m, w, 0)) return rc;
    int32_t one = 1;
    if (!put(m, m->S.reset + w, &one, 4))
        return fail(MPENV_ERR_HIP, "hipMemcpy failed");
    return MPENV_OK;
}

int mpenv_set_pvp_action(mpenv_manager *m, int32_t w, int32_t a, const int32_t discrete[4], const float aim[2],
                         const int32_t aim_discrete[2])
{
    if (int rc = checkAgent(m, w, a)) return rc;
    const int64_t g = (int64_t)w * m->S.N + a;
    bool ok = true;
    if (discrete) ok &= put(m, m->S.discreteAction + 4 * g, discrete, 16);
    if (aim) ok &= put(m, m->S.aimAction + 2 * g, aim, 8);
    if (aim_discrete) ok &= put(m, m->S.discreteAim + 2 * g, aim_discrete, 8);
    return ok ? MPENV_OK : fail(MPENV_ERR_HIP, "hipMemcpy failed");
}

int mpenv_set_hp(mpenv_manager *m, int32_t w, int32_t a, int32_t hp)
{
    if (int rc = checkAgent(m, w, a)) return rc;
    float v = (float)hp;
    if (!put(m, m->S.hp + (int64_t)w * m->S.N + a, &v, 4))
        return fail(MPENV_ERR_HIP, "hipMemcpy failed");
    return MPENV_OK;
}

int mpenv_set_agent_policy(mpenv_manager *m, int32_t w, int32_t a, int32_t policy)
{
    if (int rc = checkAgent(m, w, a)) return rc;
    if (!put(m, m->S.policy + (int64_t)w * m->S.N + a, &policy, 4))
        return fail(MPENV_ERR_HIP, "hipMemcpy failed");
    return MPENV_OK;
}

int mpenv_set_uniform_agent_policy(mpenv_manager *m, int32_t policy)
{
    if (!m) return fail(MPENV_ERR_INVALID, "null manager");
    if (hipMemsetD32Async((hipDeviceptr_t)m->S.policy, policy, (size_t)m->S.A, m->stream) != hipSuccess ||
        hipStreamSynchronize(m->stream) != hipSuccess)
        return fail(MPENV_ERR_HIP, "hipMemsetD32 failed");
    return MPENV_OK;
}

// Manager::isReplayFinished (mgr.cpp:2603-2617): the replay file hit EOF
int mpenv_is_replay_finished(mpenv_manager *m, int32_t *finished)
{
    if (!m || !finished) return fail(MPENV_ERR_INVALID, "null argument");
    if (!m->replayFile) return fail(MPENV_ERR_INVALID, "no replay log configured");
    if (!m->replayEof) {
        const int c = std::fgetc(m->replayFile);
        if (c == EOF) m->replayEof = true;
        else std::ungetc(c, m->replayFile);
    }
    *finished = m->replayEof ? 1 : 0;
    return MPENV_OK;
}

int mpenv_dims(mpenv_manager *m, int32_t *num_worlds, int32_t *agents_per_world)
{
    if (!m) return fail(MPENV_ERR_INVALID, "null manager");
    if (num_worlds) *num_worlds = m->S.W;
    if (agents_per_world) *agents_per_world = m->S.N;
    return MPENV_OK;
}

int mpenv_enable_kernel_timing(mpenv_manager *m, int32_t enable)
{
    if (!m) return fail(MPENV_ERR_INVALID, "null manager");
    m->timing = enable != 0;
    m->eventsUsed = 0;
    return MPENV_OK;
}

int mpenv_enable_stats(mpenv_manager *m, int32_t enable)
{
    if (!m) return fail(MPENV_ERR_INVALID, "null manager");
    return guarded([&] {
        HIP_CHECK(hipStreamSynchronize(m->stream));
        for (const SideStream &g : m->gside) HIP_CHECK(hipStreamSynchronize(g.stream));
        if (enable && !m->statsBuf) m->statsBuf = m->alloc<unsigned long long>(kNumStats);
        if (enable) HIP_CHECK(hipMemsetAsync(m->statsBuf, 0, sizeof(unsigned long long) * kNumStats, m->stream));
        HIP_CHECK(hipStreamSynchronize(m->stream));
        m->setStats(enable ? m->statsBuf : nullptr);
    });
}

int mpenv_read_stats(mpenv_manager *m, uint64_t *out, int32_t n)
{
    if (!m || !out) return fail(MPENV_ERR_INVALID, "null argument");
    return guarded([&] {
        std::vector<unsigned long long> h(kNumStats, 0ull);
        HIP_CHECK(hipDeviceSynchronize());
        if (m->statsBuf)
            HIP_CHECK(hipMemcpy(h.data(), m->statsBuf, sizeof(unsigned long long) * kNumStats,
                                hipMemcpyDeviceToHost));
        for (int k = 0; k < n && k < kNumStats; k++) out[k] = h[k];
        return (int)kNumStats;
    });
}

int mpenv_kernel_timings(mpenv_manager *m, int32_t max_n, const char **names, float *avg_ms, int32_t *launches)
{
    if (!m) return fail(MPENV_ERR_INVALID, "null manager");
    return guarded([&] {
        const int nk = kNumTimedKernels;
        std::vector<double> sum(nk, 0.0);
        int steps = 0;
        HIP_CHECK(hipDeviceSynchronize());
        // events per step: nk + 1 boundaries
        const size_t per = (size_t)nk + 1;
        for (size_t base = 0; base + per <= m->eventsUsed; base += per) {
            for (int k = 0; k < nk; k++) {
                float ms = 0.f;
                HIP_CHECK(hipEventElapsedTime(&ms, m->eventPool[base + k], m->eventPool[base + k + 1]));
                sum[k] += ms;
            }
            steps++;
        }
        // one segment per range and step: each kernel's time is summed over
        // the ranges (world groups, each a segment too, are not divided out)
        steps /= (int)m->ranges.size();
        m->eventsUsed = 0;
        for (int k = 0; k < nk && k < max_n; k++) {
            if (names) names[k] = kernelName(k);
            if (avg_ms) avg_ms[k] = steps ? (float)(sum[k] / steps) : 0.f;
            if (launches) launches[k] = steps;
        }
        return nk;
    });
}

} // extern "C"
