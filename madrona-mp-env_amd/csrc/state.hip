// state.hip — world checkpoints: save the batch's state, restore or fork
// chosen worlds (include/mpenv.h mpenv_state_*).
//
// A snapshot is a byte blob without pointers: a 256-B StateHeader, then one
// section per state buffer in declaration order, each at a multiple of
// 256 B.  A section holds the buffer's rows for all worlds in world order
// with the live buffer's row layout, so world s's rows are one contiguous
// span of every section and a load may take any snapshot world into any live
// world (worlds never read each other, manager.cpp sliceState).  The sections
// are the expansion of MP_AGENT_F32 / MP_AGENT_I32 / MP_WORLD_I32 /
// MP_WORLD_F32, the six columns of dmg, the buffer table MP_BUFS less the
// exemptions below, and resetKeys.  Exported observation / lidar rows and
// the input columns are inside, so every export is right directly after a
// load; visOcc (a hint only) is inside too, so a restored world also repeats
// the traversal work of the one it was saved from.
//
// Kernels, over a device-resident descriptor table (StateTab, engine.h):
//   k_state_copy      save and full load: every section streamed in one
//                     launch, 16 B per lane, kCopyInFlight loads in flight
//                     per lane, byte tail by the section's first block;
//   k_state_check     one block: the blob's header against the manager's,
//                     the world map's range; writes the go word;
//   k_state_load_map  narrow sections lane -> (world, element) along the
//                     destination; wide sections a wave per kWideWorlds
//                     destination worlds, one world span at a time.
// Loads read the go word first: a refused load writes nothing, and the host
// never synchronises.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "engine.h"
#include "mpenv_core.h"

namespace mpenv {

namespace {

// ---- which table buffers a snapshot holds.  Every MP_BUFS entry is named
// in exactly one of these two lists (checked at compile time below): a new
// buffer is one line in engine.h plus a decision here.
constexpr const char *kStateIncluded[] = {
    "visMask", "visOcc", "exploreBits", "filtLast", "zoneStats", "spawnTrack", "crumbs",
    "reset", "worldCurr", "matchResult", "exploreAction", "discreteAction", "aimAction", "discreteAim",
    "policy", "botAction", "reward", "done", "selfObs", "filters", "tmObs", "oppObs", "lkObs", "selfPos",
    "tmPos", "oppPos", "lkPos", "masks", "fwdLidar", "rearLidar", "hp", "alive", "magazine", "rewardCoefs",
    "ftActions", "ftGlobal", "ftPlayers", "ftEnemies", "ftLastKnown", "ftFwdLidar", "ftRearLidar",
    "ftReward", "ftDone", "ftPolicy",
};
struct StateExempt {
    const char *name, *why;
};
constexpr StateExempt kStateExempt[] = {
    { "agentMap", "never written: constant zeros, 4 KB per agent" },
    { "trainCtrl", "unsliced caller input, shared by every world" },
};
// Not table buffers, so outside by construction: stats, wireErr, wireEp,
// outTab and the record / replay / event log buffers.

constexpr bool strEq(const char *a, const char *b)
{
    while (*a && *a == *b) a++, b++;
    return *a == *b;
}
constexpr bool stateIncluded(const char *n)
{
    for (const char *s : kStateIncluded)
        if (strEq(s, n)) return true;
    return false;
}
constexpr bool stateExempt(const char *n)
{
    for (const StateExempt &e : kStateExempt)
        if (strEq(e.name, n)) return true;
    return false;
}
#define MP_DECIDED(n, ...) \
    static_assert(stateIncluded(#n) != stateExempt(#n), "table buffer " #n ": list it in kStateIncluded or kStateExempt");
MP_BUFS(MP_DECIDED, MP_DECIDED)
#undef MP_DECIDED

struct Sec {
    const char *name;
    int32_t kind, dtype, exportId, member, dmgCol;
    int64_t rowBytes;
};

// MPENV_DTYPE_* of a buffer's elements (float4 rows are f32, RandKey rows u32)
template <typename T>
constexpr int32_t stateDtype()
{
    return std::is_same<T, float>::value || std::is_same<T, float4>::value ? MPENV_DTYPE_FLOAT32
           : std::is_same<T, int32_t>::value                               ? MPENV_DTYPE_INT32
           : std::is_same<T, uint8_t>::value                               ? MPENV_DTYPE_UINT8
           : std::is_same<T, uint16_t>::value                              ? MPENV_DTYPE_UINT16
           : std::is_same<T, uint64_t>::value                              ? MPENV_DTYPE_UINT64
                                                                           : MPENV_DTYPE_UINT32;
}

// the sections in blob order, for team size T and spawn track length trackLen
std::vector<Sec> stateSecs(int64_t T, int64_t trackLen)
{
    std::vector<Sec> v;
#define MP_SEC_AF(n) v.push_back({ #n, kPerAgent, MPENV_DTYPE_FLOAT32, -1, (int32_t)offsetof(DevState, n), -1, 4 });
#define MP_SEC_AI(n) v.push_back({ #n, kPerAgent, MPENV_DTYPE_INT32, -1, (int32_t)offsetof(DevState, n), -1, 4 });
#define MP_SEC_WI(n) v.push_back({ #n, kPerWorld, MPENV_DTYPE_INT32, -1, (int32_t)offsetof(DevState, n), -1, 4 });
#define MP_SEC_WF(n) v.push_back({ #n, kPerWorld, MPENV_DTYPE_FLOAT32, -1, (int32_t)offsetof(DevState, n), -1, 4 });
    MP_AGENT_F32(MP_SEC_AF)
    MP_AGENT_I32(MP_SEC_AI)
    MP_WORLD_I32(MP_SEC_WI)
    MP_WORLD_F32(MP_SEC_WF)
#undef MP_SEC_AF
#undef MP_SEC_AI
#undef MP_SEC_WI
#undef MP_SEC_WF
    static const char *const dmgNames[kMaxTeamSize] = { "dmg0", "dmg1", "dmg2", "dmg3", "dmg4", "dmg5" };
    for (int k = 0; k < kMaxTeamSize; k++)
        v.push_back({ dmgNames[k], kPerAgent, MPENV_DTYPE_FLOAT32, -1, (int32_t)offsetof(DevState, dmg), k, 4 });
    // the export's name: its MPENV_EXPORT_* id without the prefix
#define MP_SEC(n, type, kind, ...) \
    if (stateIncluded(#n))         \
        v.push_back({ #n, kind, stateDtype<type>(), -1, (int32_t)offsetof(DevState, n), -1, (int64_t)sizeof(type) * rowElems(__VA_ARGS__) });
#define MP_SEC_E(n, type, kind, id, ...) \
    if (stateIncluded(#n))               \
        v.push_back({ &#id[sizeof("MPENV_EXPORT_") - 1], kind, stateDtype<type>(), id, (int32_t)offsetof(DevState, n), -1, (int64_t)sizeof(type) * rowElems(__VA_ARGS__) });
    MP_BUFS(MP_SEC, MP_SEC_E)
#undef MP_SEC
#undef MP_SEC_E
    v.push_back({ "resetKeys", kPerAgent, MPENV_DTYPE_UINT32, -1, (int32_t)offsetof(DevState, resetKeys), -1, (int64_t)sizeof(mp::RandKey) * 11 });
    return v;
}

int64_t align256(int64_t n) { return (n + 255) / 256 * 256; }

int checkS(hipError_t e) { return e == hipSuccess ? 0 : -1; }

} // namespace

int stateNumSections() { return (int)stateSecs(1, kMinSpawnTrack).size(); }

bool stateSection(int idx, int64_t W, int64_t N, int64_t trackLen, StateSectionInfo &out)
{
    const std::vector<Sec> v = stateSecs(N / 2, trackLen);
    if (idx < 0 || idx >= (int)v.size()) return false;
    int64_t off = sizeof(StateHeader);
    for (int k = 0;; k++) {
        const int64_t bytes = bufRows((RowKind)v[k].kind, W, N) * v[k].rowBytes;
        if (k == idx) {
            out = { v[k].name, off, bytes, (int32_t)v[k].rowBytes, v[k].kind, v[k].exportId, v[k].dtype,
                    v[k].member, v[k].dmgCol };
            return true;
        }
        off = align256(off + bytes);
    }
}

int64_t stateBytes(int64_t W, int64_t N, int64_t trackLen)
{
    StateSectionInfo last;
    stateSection(stateNumSections() - 1, W, N, trackLen, last);
    return last.offset + last.bytes;
}

constexpr int kCopyPieces = 8;
constexpr int kCopyInFlight = 4;
constexpr int kCopyBlockPieces = 256 * kCopyPieces;
// mapped load: a section whose span per world is at least this many bytes is
// copied a world span at a time by whole waves; below it a lane per element
constexpr int kWideSpan = 512;
constexpr int kWidePieces = 4;
constexpr int kWideWorlds = 16; // destination worlds per wave of a wide section

void buildStateTab(const DevState &s, const SceneDev &sc, StateTab *dev, StateTab &host)
{
    std::memset(&host, 0, sizeof(host));
    const int n = stateNumSections();
    if (n + 1 > kMaxStateSegs) throw std::runtime_error("state snapshot: more sections than kMaxStateSegs");
    StateHeader &h = host.hdr;
    h.magic = kStateMagic;
    h.version = kStateVersion;
    h.W = s.W;
    h.N = s.N;
    h.T = s.T;
    h.spawnTrackLen = sc.spawnTrackLen;
    h.simFlags = sc.simFlags;
    h.task = sc.task;
    h.bytes = stateBytes(s.W, s.N, sc.spawnTrackLen);
    h.sections = n;
    host.nSeg = n + 1;
    host.W = s.W;
    auto pow2 = [](uint64_t v) {
        int g = 16;
        while (g > 1 && (v & (uint64_t)(g - 1))) g >>= 1;
        return g;
    };
    int64_t first = 0, firstNarrow = 0;
    host.wideBlocks = ((int64_t)s.W + 4 * kWideWorlds - 1) / (4 * kWideWorlds);
    for (int k = 0; k <= n; k++) {
        StateSeg &g = host.seg[k];
        if (k == 0) {
            // the header: saved from the table's own copy, never loaded
            g.live = reinterpret_cast<char *>(&dev->hdr);
            g.off = 0;
            g.bytes = g.span = sizeof(StateHeader);
        } else {
            StateSectionInfo si;
            stateSection(k - 1, s.W, s.N, sc.spawnTrackLen, si);
            char *p = nullptr;
            std::memcpy(&p, reinterpret_cast<const char *>(&s) + si.member, sizeof(p));
            if (!p) throw std::runtime_error(std::string("state snapshot: buffer ") + si.name + " is not allocated");
            if (si.dmgCol >= 0) p += (int64_t)si.dmgCol * s.dmgStride * (int64_t)sizeof(float);
            g.live = p;
            g.off = si.offset;
            g.bytes = si.bytes;
            g.span = (int32_t)(si.bytes / s.W);
        }
        g.gran = pow2((uint64_t)g.span | (uint64_t)(uintptr_t)g.live);
        host.first[k] = first;
        const int64_t pieces = ((uintptr_t)g.live & 15u) ? g.bytes / g.gran : (g.bytes + 15) / 16;
        first += std::max<int64_t>(1, (pieces + kCopyBlockPieces - 1) / kCopyBlockPieces);
        if (k == 0) continue;
        if (g.span >= kWideSpan) {
            host.wideSeg[host.nWide++] = k;
        } else {
            host.narrowSeg[host.nNarrow] = k;
            host.firstNarrow[host.nNarrow++] = firstNarrow;
            firstNarrow += (g.bytes / g.gran + 255) / 256;
        }
    }
    host.first[n + 1] = first;
    host.firstNarrow[host.nNarrow] = firstNarrow;
    host.blocks = first;
    host.blocksMap = host.nWide * host.wideBlocks + firstNarrow;
    if (host.blocks >= 0x7fffffff || host.blocksMap >= 0x7fffffff)
        throw std::runtime_error("state snapshot: too many blocks for one launch");
}

// the entry of the ascending list first[lo..hi] block b falls under: the last
// one that is <= b (wave-uniform: every lane of the block walks the same path)
__device__ __forceinline__ int stateFind(const int64_t *first, int lo, int hi, int64_t b)
{
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first[mid] <= b) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// A block's kCopyBlockPieces pieces: each wave owns a contiguous run of
// them (a lane's kCopyPieces pieces 64 apart) and moves it in rounds of
// kCopyInFlight loads, then their stores.  Measured at C3 (1.47 GB): 0.52 ms
// for the save; with all 8 pieces in flight 0.79 ms, with the block's lanes
// striding together (pieces 256 apart) 0.53 ms.
template <typename V>
__device__ __forceinline__ void copyPieces(V *dst, const V *src, int64_t base, int64_t n)
{
    const int64_t p0 = base + (threadIdx.x >> 6) * (64 * kCopyPieces) + (threadIdx.x & 63);
#pragma unroll
    for (int r = 0; r < kCopyPieces; r += kCopyInFlight) {
        V v[kCopyInFlight];
#pragma unroll
        for (int j = 0; j < kCopyInFlight; j++) {
            const int64_t p = p0 + (r + j) * 64;
            if (p < n) v[j] = src[p];
        }
#pragma unroll
        for (int j = 0; j < kCopyInFlight; j++) {
            const int64_t p = p0 + (r + j) * 64;
            if (p < n) dst[p] = v[j];
        }
    }
}

// Save (load == 0: live -> blob, header included) and full load (load == 1:
// blob -> live, from segment 1 on, only when k_state_check said go).  Each
// segment has blocks of its own (StateTab::first) of kCopyBlockPieces 16-B
// pieces, every load and store instruction unit-stride.
// A segment whose live address is not 16-B aligned (the dmg columns of a
// batch of a few agents) goes in pieces of its granularity instead.
__global__ void __launch_bounds__(256) k_state_copy(StateTab *tab, char *blob, int load, int64_t skip)
{
    if (load && !*(volatile uint32_t *)&tab->go) return;
    const int64_t b = (int64_t)blockIdx.x + skip;
    const int k = stateFind(tab->first, load ? 1 : 0, tab->nSeg - 1, b);
    const StateSeg sg = tab->seg[k];
    const int64_t first = tab->first[k];
    char *bp = blob + sg.off;
    char *dst = load ? sg.live : bp;
    const char *src = load ? bp : sg.live;
    const int64_t base = (b - first) * kCopyBlockPieces;
    if (((uintptr_t)sg.live & 15u) == 0) {
        const int64_t n16 = sg.bytes / 16;
        copyPieces(reinterpret_cast<uint4 *>(dst), reinterpret_cast<const uint4 *>(src), base, n16);
        // the partial last piece (bytes % 16), by the segment's first block
        if (b == first && (int64_t)threadIdx.x < (sg.bytes & 15)) dst[n16 * 16 + threadIdx.x] = src[n16 * 16 + threadIdx.x];
    } else {
        const int64_t n = sg.bytes / sg.gran;
        switch (sg.gran) {
        case 8: copyPieces(reinterpret_cast<uint2 *>(dst), reinterpret_cast<const uint2 *>(src), base, n); break;
        case 4: copyPieces(reinterpret_cast<uint32_t *>(dst), reinterpret_cast<const uint32_t *>(src), base, n); break;
        case 2: copyPieces(reinterpret_cast<uint16_t *>(dst), reinterpret_cast<const uint16_t *>(src), base, n); break;
        default: copyPieces(reinterpret_cast<uint8_t *>(dst), reinterpret_cast<const uint8_t *>(src), base, n); break;
        }
    }
}

// One block.  The blob's header must equal this manager's byte for byte
// (magic, version, W, N, T, track length, flags, task, bytes, sections and
// the reserved words: zeros, or a map set's layout hash); every map entry
// must be -1 or a world, and on a map-set manager a world of the same scene
// as its destination (MPENV_STATE_ERR_CROSS_MAP).  go = 1 only when all
// hold; otherwise the error bits are raised and the load that follows on the
// stream returns at once.
__global__ void __launch_bounds__(256) k_state_check(StateTab *tab, const char *src, const int32_t *map)
{
    __shared__ uint32_t bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    uint32_t mine = 0;
    if (threadIdx.x < sizeof(StateHeader) / 4 &&
        reinterpret_cast<const uint32_t *>(src)[threadIdx.x] != reinterpret_cast<const uint32_t *>(&tab->hdr)[threadIdx.x])
        mine |= MPENV_STATE_ERR_HEADER;
    if (map) {
        // four 16-B loads in flight per lane (the map is 16-B aligned); this
        // one block is on the critical path of every mapped load
        const int32_t W = tab->W;
        const int32_t n4 = W / 4;
        const int4 *m4 = reinterpret_cast<const int4 *>(map);
        auto outside = [W](int32_t s) { return s < -1 || s >= W; };
        // map sets: world d may take snapshot world s only when both play the
        // same scene (the blob's range layout is this manager's: the header
        // check); the table reads follow the range check of s
        const int32_t *mow = tab->mapOfWorld;
        // the table is handed out (mpenv_map_of_world): an entry a caller
        // overwrote still indexes inside rangeScene
        auto sceneOf = [mow, tab](int32_t w) { return tab->rangeScene[(uint32_t)mow[w] % MPENV_MAX_MAP_RANGES]; };
        auto crossMap = [sceneOf](int32_t d, int32_t s) { return sceneOf(d) != sceneOf(s); };
        auto entry = [&](int32_t d, int32_t s) -> uint32_t {
            if (outside(s)) return MPENV_STATE_ERR_MAP;
            return mow && s >= 0 && crossMap(d, s) ? MPENV_STATE_ERR_CROSS_MAP : 0u;
        };
        for (int32_t base = 0; base < n4; base += 4 * 256) {
            int4 v[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int32_t i = base + j * 256 + (int32_t)threadIdx.x;
                v[j] = i < n4 ? m4[i] : make_int4(-1, -1, -1, -1);
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                // -1 for the lanes past n4: never a table read
                const int32_t d0 = 4 * (base + j * 256 + (int32_t)threadIdx.x);
                mine |= entry(d0, v[j].x) | entry(d0 + 1, v[j].y) | entry(d0 + 2, v[j].z) | entry(d0 + 3, v[j].w);
            }
        }
        const int32_t d = n4 * 4 + (int32_t)threadIdx.x; // W % 4 entries left
        if (d < W) mine |= entry(d, map[d]);
    }
    if (mine) atomicOr(&bad, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        tab->go = bad == 0;
        if (bad) atomicOr(&tab->err, bad);
    }
}

template <typename V>
__device__ __forceinline__ void copyWide(char *dst, const char *src, int n, int lane)
{
    V *d = reinterpret_cast<V *>(dst);
    const V *s = reinterpret_cast<const V *>(src);
    for (int e0 = lane; e0 < n; e0 += 64 * kWidePieces) {
        V v[kWidePieces];
#pragma unroll
        for (int j = 0; j < kWidePieces; j++)
            if (e0 + 64 * j < n) v[j] = s[e0 + 64 * j];
#pragma unroll
        for (int j = 0; j < kWidePieces; j++)
            if (e0 + 64 * j < n) d[e0 + 64 * j] = v[j];
    }
}

template <typename V>
__device__ __forceinline__ void copyElem(char *dst, const char *src)
{
    *reinterpret_cast<V *>(dst) = *reinterpret_cast<const V *>(src);
}

// Mapped load: live world d <- snapshot world map[d]; -1 keeps d.  Worlds are
// disjoint destinations, so no atomics.  Elements are `gran` bytes (up to 16).
//   narrow  lane -> (world, element) along the destination column: stores
//           coalesce whatever the map is, loads for identity-like maps;
//   wide    a wave per kWideWorlds destination worlds, each restored span
//           copied 64 elements per instruction, kWidePieces loads in
//           flight; kept worlds are skipped before any load of theirs.
__global__ void __launch_bounds__(256) k_state_load_map(StateTab *tab, const char *blob, const int32_t *map, int32_t W,
                                                        int64_t wideBlocks, int64_t allWide)
{
    const int64_t b = blockIdx.x;
    if (b < allWide) {
        // wide sections first, wideBlocks blocks each: the section and the
        // worlds come from the block index alone.  A wave owns kWideWorlds
        // consecutive destination worlds: one load fetches their map
        // entries, and a wave whose worlds are all kept leaves having read
        // nothing else (a wave per world was ~400,000 waves at C3, each
        // waiting out one load's latency: 0.12 ms for a 1 % load)
        const int64_t kw = b / wideBlocks;
        const int64_t d0 = ((b - kw * wideBlocks) * 4 + (threadIdx.x >> 6)) * kWideWorlds;
        const int lane = threadIdx.x & 63;
        int32_t s = -1;
        if (lane < kWideWorlds && d0 + lane < W) s = map[d0 + lane];
        if (!*(volatile uint32_t *)&tab->go) return;
        unsigned long long todo = __ballot(s >= 0);
        if (!todo) return;
        const StateSeg sg = tab->seg[tab->wideSeg[kw]];
        const int epw = sg.span / sg.gran; // elements per world
        while (todo) {
            const int i = __ffsll(todo) - 1;
            todo &= todo - 1;
            char *dp = sg.live + (d0 + i) * sg.span;
            const char *sp = blob + sg.off + (int64_t)__shfl(s, i) * sg.span;
            switch (sg.gran) {
            case 16: copyWide<uint4>(dp, sp, epw, lane); break;
            case 8: copyWide<uint2>(dp, sp, epw, lane); break;
            case 4: copyWide<uint32_t>(dp, sp, epw, lane); break;
            case 2: copyWide<uint16_t>(dp, sp, epw, lane); break;
            default: copyWide<uint8_t>(dp, sp, epw, lane); break;
            }
        }
    } else {
        if (!*(volatile uint32_t *)&tab->go) return;
        const int64_t bn = b - allWide;
        const int j = stateFind(tab->firstNarrow, 0, tab->nNarrow - 1, bn);
        const StateSeg sg = tab->seg[tab->narrowSeg[j]];
        const int epw = sg.span / sg.gran;
        const int64_t i = (bn - tab->firstNarrow[j]) * 256 + threadIdx.x;
        if (i >= (int64_t)W * epw) return;
        const int64_t d = i / epw;
        const int64_t e = i - d * epw;
        const int32_t s = map[d];
        if (s < 0) return;
        char *dp = sg.live + i * sg.gran;
        const char *sp = blob + sg.off + ((int64_t)s * epw + e) * sg.gran;
        switch (sg.gran) {
        case 16: copyElem<uint4>(dp, sp); break;
        case 8: copyElem<uint2>(dp, sp); break;
        case 4: copyElem<uint32_t>(dp, sp); break;
        case 2: copyElem<uint16_t>(dp, sp); break;
        default: copyElem<uint8_t>(dp, sp); break;
        }
    }
}

static int launchStateCopy(const StateTab &host, StateTab *dev, char *blob, int load, hipStream_t st)
{
    const int64_t skip = load ? host.first[1] : 0;
    hipLaunchKernelGGL(k_state_copy, dim3((unsigned)(host.blocks - skip)), dim3(256), 0, st, dev, blob, load, skip);
    return checkS(hipGetLastError());
}

int launchStateSave(const StateTab &host, StateTab *dev, char *dst, void *stream)
{
    return launchStateCopy(host, dev, dst, 0, (hipStream_t)stream);
}

int launchStateLoad(const StateTab &host, StateTab *dev, const char *src, const int32_t *map, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_state_check, dim3(1), dim3(256), 0, st, dev, src, map);
    if (checkS(hipGetLastError())) return -1;
    if (!map) return launchStateCopy(host, dev, const_cast<char *>(src), 1, st);
    hipLaunchKernelGGL(k_state_load_map, dim3((unsigned)host.blocksMap), dim3(256), 0, st, dev, src, map, host.W,
                       host.wideBlocks, host.nWide * host.wideBlocks);
    return checkS(hipGetLastError());
}

} // namespace mpenv
