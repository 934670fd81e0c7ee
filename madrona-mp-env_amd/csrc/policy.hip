// policy.hip — in-sim policy inference on gfx950 (DESIGN.md §2 definition 15,
// §4 "Policy kernels"): the reference's evalAgentPolicy (src/dnn.cpp:555-891,
// CPU only there) on the step's stream: three small selection kernels, then
// the two that compute.
//
//   k_pol_count   how many agents each checkpoint slot serves (policy.h: slot
//                 p, else slot 0, else nobody): one ballot per slot present in
//                 a wave into the block's LDS histogram, one global atomic per
//                 slot present in the block
//   k_pol_plan    one wave: the 32 counts into segment bases padded to 64 list
//                 positions, and per 64-row tile its blob, live rows and slot
//   k_pol_scatter agent ids into their slot's segment (ballot + prefix in the
//                 wave, LDS atomic in the block, one global atomic per slot and
//                 block); the order inside a segment differs from run to run
//                 and no result depends on it
//   k_pol_embed   normalisation, position embedding and the 20 embeddings of
//                 four agents per wave (lane = output feature, explicit fmaf
//                 chains on the VALU); 384 floats per agent
//                 (a block's 16 list positions lie in one tile, so one slot)
//   k_pol_trunk   one tile of 64 agents per block, the blob of the tile's slot,
//                 activations resident in LDS: the three
//                 512-wide layers and both heads on v_mfma_f32_32x32x2_f32,
//                 LayerNorm statistics one row per lane, Gumbel-max sampling
//                 on the agent lanes
//
// Every dense output is one k-ascending fmaf chain from +0: the f32-input
// MFMA computes exactly that (one rounding per product, k order), K is never
// split across accumulators or waves, and zero padding of K is exact.
//
// Counts, bases and the tile tables are written by one kernel and read by the
// next: the kernel boundary on the stream is the only ordering relied on.
#include <hip/hip_runtime.h>

#include "policy.h"

namespace mpenv {

using namespace pol;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
// A checkpoint's parameters.  The blob pointer comes out of a table in memory,
// where the compiler cannot see that it points to global memory and would read
// through it with flat loads (which also count as LDS traffic and stall the
// operand prefetch behind the LDS reads); the type says it.
typedef const __attribute__((address_space(1))) float *BlobPtr;

constexpr int kTileRows = 64;       // agents per trunk block
static_assert(kTileRows == kSegAlign, "a slot's segment starts on a trunk tile");
constexpr int kLdx = 514;           // LDS row stride in floats: row r starts at bank 2 r, so the A-operand
                                    // read (32 rows x 2 adjacent k) touches 64 different banks
constexpr int kTrunkThreads = 512;  // 8 waves, 64 output columns each
constexpr size_t kTrunkLds = (size_t)(kTileRows * kLdx + kHidden + 2 * kTileRows) * sizeof(float);
constexpr size_t kDenseLds = (size_t)(kTileRows * kLdx) * sizeof(float);

constexpr int kEmbedAgents = 4;     // agents per wave of k_pol_embed
constexpr int kEmbedWaves = 4;
constexpr int kEmbedRowsMax = kEmbedAgents * kOppSlots; // 24
constexpr int kYStride = 65;
static_assert(kSegAlign % (kEmbedWaves * kEmbedAgents) == 0, "an embed block never straddles two segments");

__device__ __forceinline__ float negInf() { return mp::u2f(0xff800000u); }

// acc[mt][nt] = X[row0 + 32 mt ..][0 .. 2 ksteps) . W[.., tile nt], X in LDS
// (row stride kLdx), W packed (policy.h packB) with wp at the first tile.
// Lane l feeds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]; every
// k step accumulates into the same registers, so each output is the chain
// fma(a_k, b_k, ...) over k ascending.
template <int MT, int NT>
__device__ __forceinline__ void mfmaDense(const float *xs, int row0, int ksteps, BlobPtr wp, f32x16 (&acc)[MT][NT])
{
    constexpr int U = 8; // k steps per chunk: the next chunk's operands are loaded while this one's MFMAs run
    const int lane = threadIdx.x & 63;
    const float *xa = xs + (row0 + (lane & 31)) * kLdx + (lane >> 5);
    const BlobPtr wb = wp + lane;
    const int64_t tileStride = (int64_t)ksteps * 64;
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
#pragma unroll
            for (int v = 0; v < 16; v++) acc[mt][nt][v] = 0.f;

    float a[U][MT], b[U][NT], an[U][MT], bn[U][NT];
    auto load = [&](float (&pa)[U][MT], float (&pb)[U][NT], int s0) {
#pragma unroll
        for (int u = 0; u < U; u++) {
#pragma unroll
            for (int mt = 0; mt < MT; mt++) pa[u][mt] = xa[mt * 32 * kLdx + 2 * (s0 + u)];
#pragma unroll
            for (int nt = 0; nt < NT; nt++) pb[u][nt] = wb[nt * tileStride + (int64_t)(s0 + u) * 64];
        }
    };
    const int chunks = ksteps / U;
    if (chunks > 0) load(a, b, 0);
    for (int c = 0; c < chunks; c++) {
        // the last chunk loads itself again (no branch in the loop; the values are not used)
        load(an, bn, (c + 1 < chunks ? c + 1 : c) * U);
        __builtin_amdgcn_sched_barrier(0); // keep the loads in front of the MFMAs (the scheduler sinks them to their uses)
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int nt = 0; nt < NT; nt++)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][mt], b[u][nt], acc[mt][nt], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < U; u++) {
#pragma unroll
            for (int mt = 0; mt < MT; mt++) a[u][mt] = an[u][mt];
#pragma unroll
            for (int nt = 0; nt < NT; nt++) b[u][nt] = bn[u][nt];
        }
    }
    for (int s = chunks * U; s < ksteps; s++) { // K / 2 not a multiple of the chunk (test shapes only)
        float ta[MT], tb[NT];
#pragma unroll
        for (int mt = 0; mt < MT; mt++) ta[mt] = xa[mt * 32 * kLdx + 2 * s];
#pragma unroll
        for (int nt = 0; nt < NT; nt++) tb[nt] = wb[nt * tileStride + (int64_t)s * 64];
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int nt = 0; nt < NT; nt++)
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(ta[mt], tb[nt], acc[mt][nt], 0, 0, 0);
    }
}

// C/D map of the 32x32 MFMA: register v of lane l is row 8 (v >> 2) + 4 (l >> 5) + (v & 3), column l & 31.
template <int MT, int NT>
__device__ __forceinline__ void storeTiles(float *xs, int row0, int col0, const f32x16 (&acc)[MT][NT])
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
#pragma unroll
            for (int v = 0; v < 16; v++) {
                const int r = row0 + 32 * mt + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3);
                xs[r * kLdx + col0 + 32 * nt + (lane & 31)] = acc[mt][nt][v];
            }
}

// sampleLogits (dnn.cpp:536-553): Gumbel-max; a strictly greater score wins,
// bucket 0 if nothing beats -inf (u = 0 gives logf_(0) = -inf, so g = -inf).
__device__ int32_t sampleHead(const float *lg, int nb, mp::RandKey k)
{
    int32_t best = 0;
    float mx = negInf();
    for (int i = 0; i < nb; i++) {
        const float u = mp::keyUniform(mp::splitI(k, (uint32_t)i));
        const float g = -mp::logf_(-mp::logf_(u));
        const float score = lg[i] + g;
        if (score > mx) {
            mx = score;
            best = i;
        }
    }
    return best;
}

// ---- selection ------------------------------------------------------------

// the slot that serves policy id p while the slots of `mask` hold checkpoints, or -1
__device__ __forceinline__ int slotOf(int32_t p, uint32_t mask)
{
    if (p < 0) return -1;
    if (p < kSlots && ((mask >> p) & 1u)) return p;
    return (mask & 1u) ? 0 : -1;
}

// fn(s, lanes) once for every slot s present in the wave, lanes = who has it
template <typename F>
__device__ __forceinline__ void forEachSlotOfWave(int slot, F fn)
{
    unsigned long long rest = __ballot(slot >= 0);
    while (rest) {
        const int s = __shfl(slot, __ffsll(rest) - 1);
        const unsigned long long same = __ballot(slot == s);
        fn(s, same);
        rest &= ~same;
    }
}

constexpr int kSelThreads = 1024; // a large block: its LDS histogram leaves one global atomic per slot and block

__global__ void __launch_bounds__(kSelThreads) k_pol_count(DevState S, PolicyDev P)
{
    __shared__ int32_t hist[kSlots]; // the block's agents per slot
    if (threadIdx.x < kSlots) hist[threadIdx.x] = 0;
    __syncthreads();
    const int64_t g = (int64_t)blockIdx.x * kSelThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int slot = g < S.A ? slotOf(S.policy[g], P.mask) : -1;
    forEachSlotOfWave(slot, [&](int s, unsigned long long same) {
        if (lane == 0) atomicAdd(&hist[s], (int)__popcll(same));
    });
    __syncthreads();
    if (threadIdx.x < kSlots && hist[threadIdx.x] > 0) atomicAdd(P.count + threadIdx.x, hist[threadIdx.x]);
}

// One wave.  Every one of the numTiles tiles is written: the live ones, then rows = 0.
__global__ void __launch_bounds__(64) k_pol_plan(PolicyDev P, int numTiles)
{
    const int lane = threadIdx.x;
    const int c = lane < kSlots ? P.count[lane] : 0;
    const int padded = (c + kSegAlign - 1) / kSegAlign * kSegAlign;
    int end = padded; // inclusive prefix sum over the lanes
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(end, d);
        if (lane >= d) end += up;
    }
    const int base = end - padded;
    if (lane < kSlots) P.cursor[lane] = base;
    for (int s = 0; s < kSlots; s++) { // the tiles of segment s, a tile per lane
        const int sc = __shfl(c, s), t0 = __shfl(base, s) / kSegAlign;
        if (sc == 0) continue;
        const float *blob = P.blobs[s];
        for (int t = lane; t * kSegAlign < sc; t += 64) P.tiles[t0 + t] = Tile { blob, min(kSegAlign, sc - t * kSegAlign), s };
    }
    for (int t = __shfl(end, 63) / kSegAlign + lane; t < numTiles; t += 64) P.tiles[t] = Tile { nullptr, 0, 0 };
}

__global__ void __launch_bounds__(kSelThreads) k_pol_scatter(DevState S, PolicyDev P)
{
    __shared__ int32_t hist[kSlots]; // the block's agents per slot, then the block's base in that slot's segment
    if (threadIdx.x < kSlots) hist[threadIdx.x] = 0;
    __syncthreads();
    const int64_t g = (int64_t)blockIdx.x * kSelThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int slot = g < S.A ? slotOf(S.policy[g], P.mask) : -1;
    int at = 0; // this agent among the block's agents of its slot
    forEachSlotOfWave(slot, [&](int s, unsigned long long same) {
        int off = 0;
        if (lane == 0) off = atomicAdd(&hist[s], (int)__popcll(same));
        off = __shfl(off, 0);
        if (slot == s) at = off + (int)__popcll(same & ((1ull << lane) - 1ull));
    });
    __syncthreads();
    if (threadIdx.x < kSlots && hist[threadIdx.x] > 0)
        hist[threadIdx.x] = atomicAdd(P.cursor + threadIdx.x, hist[threadIdx.x]);
    __syncthreads();
    if (slot >= 0) P.list[hist[slot] + at] = (int32_t)g;
}

// ---- k_pol_embed -----------------------------------------------------------

// invStd * (x - mean) for `len` consecutive floats of one agent (the
// normalize*Ob functions, dnn.cpp:193-379; parameters repeat every `period`)
__device__ __forceinline__ void normSpan(BlobPtr blob, const Layout &L, const float *src, int len, int param,
                                         int period, float *dst, bool live)
{
    const int lane = threadIdx.x & 63;
    for (int e = lane; e < len; e += 64) {
        const int p = param + (e % period);
        const float x = live ? src[e] : 0.f;
        dst[e] = blob[L.normInv + p] * (x - blob[L.normMean + p]);
    }
}

template <int R>
__device__ __forceinline__ void embedDense(BlobPtr W, const float *xin, int K, float (&acc)[R])
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = 0.f;
    // the next four weights are in flight while this group's chains advance
    float w0 = W[0 * kEmbed + lane], w1 = W[1 * kEmbed + lane], w2 = W[2 * kEmbed + lane], w3 = W[3 * kEmbed + lane];
    for (int k = 0; k < K; k += 4) {
        const int kn = k + 4 < K ? k + 4 : k;
        const float n0 = W[(kn + 0) * kEmbed + lane], n1 = W[(kn + 1) * kEmbed + lane];
        const float n2 = W[(kn + 2) * kEmbed + lane], n3 = W[(kn + 3) * kEmbed + lane];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const float4 x = *reinterpret_cast<const float4 *>(xin + r * K + k);
            acc[r] = mp::fma_(w0, x.x, acc[r]);
            acc[r] = mp::fma_(w1, x.y, acc[r]);
            acc[r] = mp::fma_(w2, x.z, acc[r]);
            acc[r] = mp::fma_(w3, x.w, acc[r]);
        }
        w0 = n0;
        w1 = n1;
        w2 = n2;
        w3 = n3;
    }
}

// LayerNorm + leaky ReLU of R rows held one feature per lane
// (evalFullyConnectedLayerWithLayerNormWithActivation, dnn.cpp:428-524): the
// Welford pass over the 64 outputs in index order runs one row per lane.
template <int R>
__device__ __forceinline__ void embedNorm(float (&acc)[R], float *ybuf, float *stat, BlobPtr scale, BlobPtr bias)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int r = 0; r < R; r++) ybuf[r * kYStride + lane] = acc[r];
    __syncthreads();
    if (lane < R) {
        float mean = 0.f, m2 = 0.f;
        for (int i0 = 0; i0 < kEmbed; i0 += 16) { // 16 values per LDS wait, not one
            float y[16];
#pragma unroll
            for (int j = 0; j < 16; j++) y[j] = ybuf[lane * kYStride + i0 + j];
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const float delta = y[j] - mean;
                mean = mp::fma_(delta, 1.f / (float)(i0 + j + 1), mean);
                const float delta2 = y[j] - mean;
                m2 = mp::fma_(delta, delta2, m2);
            }
        }
        stat[2 * lane] = mean;
        stat[2 * lane + 1] = mp::sqrt_(m2 / (float)kEmbed + 1e-6f);
    }
    __syncthreads();
    const float sc = scale[lane], bs = bias[lane];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const float o = mp::fma_(sc / stat[2 * r + 1], acc[r] - stat[2 * r], bs);
        acc[r] = o >= 0.f ? o : 1e-2f * o;
    }
    __syncthreads();
}

// fwdSlot < 0: the step path, the list by tile.  Otherwise
// every agent through the checkpoint of slot fwdSlot.
__global__ void __launch_bounds__(kEmbedWaves * 64) k_pol_embed(DevState S, PolicyDev P, Layout L, int fwdSlot)
{
    constexpr int G = kEmbedAgents;
    __shared__ __attribute__((aligned(16))) float s_xin[kEmbedWaves][G * kFwdIn];
    __shared__ float s_y[kEmbedWaves][kEmbedRowsMax * kYStride];
    __shared__ float s_stat[kEmbedWaves][2 * kEmbedRowsMax];

    const bool useList = fwdSlot < 0;
    const int64_t pos0 = (int64_t)blockIdx.x * (kEmbedWaves * G);
    int64_t n = S.A; // one past the block's last live position
    BlobPtr blob;
    if (useList) {
        const int64_t tile = pos0 / kTileRows;
        const Tile t = P.tiles[tile];
        blob = (BlobPtr)t.blob;
        n = tile * kTileRows + t.rows;
    } else {
        blob = (BlobPtr)P.blobs[fwdSlot];
    }
    if (pos0 >= n) return; // the whole block (uniform): past the list, or the dead tail of a segment
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *xin = s_xin[wave], *ybuf = s_y[wave], *stat = s_stat[wave];

    int64_t pos[G], agent[G];
    bool live[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
        pos[g] = ((int64_t)blockIdx.x * kEmbedWaves + wave) * G + g;
        live[g] = pos[g] < n;
        agent[g] = live[g] ? (useList ? (int64_t)P.list[pos[g]] : pos[g]) : 0;
    }
    auto emit = [&](int g, int mod, float v) {
        if (live[g]) P.emb[pos[g] * kTrunkIn + mod * kEmbed + lane] = v;
    };

    { // self: observation, reward coefficients, position frequency embedding (dnn.cpp:593-624)
#pragma unroll
        for (int g = 0; g < G; g++) {
            float *dst = xin + g * kSelfIn;
            normSpan(blob, L, S.selfObs + agent[g] * kSelfObs, kSelfObs, kNormSelf, kSelfObs, dst, live[g]);
            normSpan(blob, L, S.rewardCoefs + agent[g] * kCoefs, kCoefs, kNormCoefs, kCoefs, dst + kSelfObs, live[g]);
            if (lane < 6 * kPosFreqs) { // positionFrequencyEmbedding (dnn.cpp:381-406): sin rows before cos rows
                const int f = lane / 6, rem = lane % 6;
                const float p = live[g] ? S.selfPos[agent[g] * 3 + rem % 3] : 0.f;
                const float scaled = p * (float)(1 << f) * mp::kPi;
                dst[kSelfObs + kCoefs + lane] = rem < 3 ? mp::sinf_(scaled) : mp::cosf_(scaled);
            }
        }
        __syncthreads();
        float acc[G];
        embedDense<G>(blob + L.embedW[kModSelf], xin, kSelfIn, acc);
        embedNorm<G>(acc, ybuf, stat, blob + L.embedScale[kModSelf], blob + L.embedBias[kModSelf]);
#pragma unroll
        for (int g = 0; g < G; g++) emit(g, kModSelf, acc[g]);
    }
    { // forward lidar (dnn.cpp:626-636)
#pragma unroll
        for (int g = 0; g < G; g++)
            normSpan(blob, L, S.fwdLidar + agent[g] * kFwdIn, kFwdIn, kNormFwd, 4, xin + g * kFwdIn, live[g]);
        __syncthreads();
        float acc[G];
        embedDense<G>(blob + L.embedW[kModFwd], xin, kFwdIn, acc);
        embedNorm<G>(acc, ybuf, stat, blob + L.embedScale[kModFwd], blob + L.embedBias[kModFwd]);
#pragma unroll
        for (int g = 0; g < G; g++) emit(g, kModFwd, acc[g]);
    }
    { // rear lidar (dnn.cpp:638-648)
#pragma unroll
        for (int g = 0; g < G; g++)
            normSpan(blob, L, S.rearLidar + agent[g] * kRearIn, kRearIn, kNormRear, 4, xin + g * kRearIn, live[g]);
        __syncthreads();
        float acc[G];
        embedDense<G>(blob + L.embedW[kModRear], xin, kRearIn, acc);
        embedNorm<G>(acc, ybuf, stat, blob + L.embedScale[kModRear], blob + L.embedBias[kModRear]);
#pragma unroll
        for (int g = 0; g < G; g++) emit(g, kModRear, acc[g]);
    }
    { // teammates: all 5 slots whatever the team size, max from -inf (dnn.cpp:650-672)
        constexpr int R = G * kTmSlots;
#pragma unroll
        for (int g = 0; g < G; g++)
            normSpan(blob, L, S.tmObs + agent[g] * (kTmSlots * kOtherObs), kTmSlots * kOtherObs, kNormTm, kOtherObs,
                     xin + g * kTmSlots * kOtherObs, live[g]);
        __syncthreads();
        float acc[R];
        embedDense<R>(blob + L.embedW[kModTm], xin, kOtherObs, acc);
        embedNorm<R>(acc, ybuf, stat, blob + L.embedScale[kModTm], blob + L.embedBias[kModTm]);
#pragma unroll
        for (int g = 0; g < G; g++) {
            float cur = negInf();
#pragma unroll
            for (int s = 0; s < kTmSlots; s++) cur = mp::fmaxD(cur, acc[g * kTmSlots + s]);
            emit(g, kModTm, cur);
        }
    }
    { // opponents: the slot's embedding times its mask before the max (dnn.cpp:674-700)
        constexpr int R = G * kOppSlots;
#pragma unroll
        for (int g = 0; g < G; g++)
            normSpan(blob, L, S.oppObs + agent[g] * (kOppSlots * kOtherObs), kOppSlots * kOtherObs, kNormOpp, kOtherObs,
                     xin + g * kOppSlots * kOtherObs, live[g]);
        __syncthreads();
        float acc[R];
        embedDense<R>(blob + L.embedW[kModOpp], xin, kOtherObs, acc);
        embedNorm<R>(acc, ybuf, stat, blob + L.embedScale[kModOpp], blob + L.embedBias[kModOpp]);
#pragma unroll
        for (int g = 0; g < G; g++) {
            float cur = negInf();
#pragma unroll
            for (int s = 0; s < kOppSlots; s++) {
                const float mask = live[g] ? S.masks[agent[g] * kOppSlots + s] : 0.f;
                cur = mp::fmaxD(cur, mask * acc[g * kOppSlots + s]);
            }
            emit(g, kModOpp, cur);
        }
    }
    { // last-known opponents (dnn.cpp:702-726)
        constexpr int R = G * kOppSlots;
#pragma unroll
        for (int g = 0; g < G; g++)
            normSpan(blob, L, S.lkObs + agent[g] * (kOppSlots * kOtherObs), kOppSlots * kOtherObs, kNormLk, kOtherObs,
                     xin + g * kOppSlots * kOtherObs, live[g]);
        __syncthreads();
        float acc[R];
        embedDense<R>(blob + L.embedW[kModLk], xin, kOtherObs, acc);
        embedNorm<R>(acc, ybuf, stat, blob + L.embedScale[kModLk], blob + L.embedBias[kModLk]);
#pragma unroll
        for (int g = 0; g < G; g++) {
            float cur = negInf();
#pragma unroll
            for (int s = 0; s < kOppSlots; s++) cur = mp::fmaxD(cur, acc[g * kOppSlots + s]);
            emit(g, kModLk, cur);
        }
    }
}

// ---- k_pol_trunk -----------------------------------------------------------

// fwdSlot < 0: the step path (tile blockIdx.x of P.list, the blob of its slot,
// actions into the engine's columns, RNG advanced by 6).  Otherwise every
// agent through slot fwdSlot, logits / actions into the caller's buffers and
// no engine state written.
__global__ void __launch_bounds__(kTrunkThreads) k_pol_trunk(DevState S, PolicyDev P, Layout L, int fwdSlot,
                                                             float *logitsOut, int32_t *actionsOut)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *xs = lds;                          // [64][kLdx] activations
    float *rcp = lds + kTileRows * kLdx;      // 1 / (i + 1)
    float *stat = rcp + kHidden;              // mean, sigma per row

    const bool useList = fwdSlot < 0;
    const int64_t base = (int64_t)blockIdx.x * kTileRows;
    int64_t n = S.A; // one past the tile's last live row
    BlobPtr blob;
    if (useList) {
        const Tile t = P.tiles[blockIdx.x];
        blob = (BlobPtr)t.blob;
        n = base + t.rows;
    } else {
        blob = (BlobPtr)P.blobs[fwdSlot];
    }
    if (base >= n) return; // past the list
    const int tid = threadIdx.x, wave = tid >> 6;

    rcp[tid] = 1.f / (float)(tid + 1);
    for (int idx = tid; idx < kTileRows * kTrunkIn; idx += kTrunkThreads) {
        const int r = idx / kTrunkIn, c = idx - r * kTrunkIn;
        xs[r * kLdx + c] = base + r < n ? P.emb[(base + r) * kTrunkIn + c] : 0.f;
    }
    __syncthreads();

    for (int layer = 0; layer < 3; layer++) {
        const int ksteps = (layer == 0 ? kTrunkIn : kHidden) / 2;
        f32x16 acc[2][2];
        mfmaDense<2, 2>(xs, 0, ksteps, blob + L.trunkW[layer] + (int64_t)(2 * wave) * ksteps * 64, acc);
        __syncthreads(); // every wave has read its inputs
        storeTiles<2, 2>(xs, 0, 64 * wave, acc);
        __syncthreads();
        if (tid < kTileRows) { // Welford over the 512 outputs in index order (dnn.cpp:438-460)
            const float *y = xs + tid * kLdx;
            float mean = 0.f, m2 = 0.f;
            for (int i0 = 0; i0 < kHidden; i0 += 16) { // 16 values and reciprocals per LDS wait, not one
                float v[16], rc[16];
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    v[j] = y[i0 + j];
                    rc[j] = rcp[i0 + j];
                }
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    const float delta = v[j] - mean;
                    mean = mp::fma_(delta, rc[j], mean);
                    const float delta2 = v[j] - mean;
                    m2 = mp::fma_(delta, delta2, m2);
                }
            }
            stat[2 * tid] = mean;
            stat[2 * tid + 1] = mp::sqrt_(m2 / (float)kHidden + 1e-6f);
        }
        __syncthreads();
        { // column tid of every row (dnn.cpp:513-523, slope 0)
            const float sc = blob[L.trunkScale[layer] + tid], bs = blob[L.trunkBias[layer] + tid];
            for (int r = 0; r < kTileRows; r++) {
                const float o = mp::fma_(sc / stat[2 * r + 1], xs[r * kLdx + tid] - stat[2 * r], bs);
                xs[r * kLdx + tid] = o >= 0.f ? o : 0.f * o;
            }
        }
        __syncthreads();
    }

    // both heads as one 512 x 64 dense: four waves, one 32 x 32 tile each
    f32x16 hacc[1][1];
    const int mt = wave & 1, nt = (wave >> 1) & 1;
    if (wave < 4) mfmaDense<1, 1>(xs, 32 * mt, kHidden / 2, blob + L.headW + (int64_t)nt * (kHidden / 2) * 64, hacc);
    __syncthreads();
    if (wave < 4) storeTiles<1, 1>(xs, 32 * mt, 32 * nt, hacc);
    __syncthreads();

    if (tid >= kTileRows || base + tid >= n) return;
    const int64_t g = useList ? (int64_t)P.list[base + tid] : base + tid;
    float *lg = xs + tid * kLdx; // the agent's own row
    for (int j = 0; j < kLogits; j++) lg[j] = lg[j] + blob[L.headBias + j];
    if (logitsOut)
        for (int j = 0; j < kLogits; j++) logitsOut[g * kLogits + j] = lg[j];
    if (!useList && !actionsOut) return;

    // moveAmount, moveAngle, fire, stand, yaw, pitch: one rngAdvance each (dnn.cpp:796-840)
    constexpr int kBuckets[kNumHeads] = { 3, 8, 3, 3, 13, 7 };
    mp::RNG rng;
    rng.key.a = (uint32_t)S.rngA[g];
    rng.key.b = (uint32_t)S.rngB[g];
    rng.ctr = (uint32_t)S.rngCtr[g];
    int32_t act[kNumHeads];
    int at = 0;
#pragma unroll
    for (int h = 0; h < kNumHeads; h++) {
        act[h] = sampleHead(lg + at, kBuckets[h], mp::rngAdvance(rng));
        at += kBuckets[h];
    }
    if (useList) {
        reinterpret_cast<int4 *>(S.discreteAction)[g] = make_int4(act[0], act[1], act[2], act[3]);
        reinterpret_cast<int2 *>(S.discreteAim)[g] = make_int2(act[4], act[5]);
        S.rngCtr[g] = (int32_t)rng.ctr;
    } else {
        for (int h = 0; h < kNumHeads; h++) actionsOut[g * kNumHeads + h] = act[h];
    }
}

// mpenv_debug_policy_dense: one wave per 64 x 64 output tile through mfmaDense
__global__ void __launch_bounds__(64) k_pol_dense(const float *x, int M, int K, const float *wp, int N, float *y)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kTileRows;
    const int Kp = (K + 1) & ~1;
    for (int idx = lane; idx < kTileRows * Kp; idx += 64) {
        const int r = idx / Kp, c = idx - r * Kp;
        lds[r * kLdx + c] = (row0 + r < M && c < K) ? x[(row0 + r) * K + c] : 0.f;
    }
    __syncthreads();
    f32x16 acc[2][2];
    mfmaDense<2, 2>(lds, 0, Kp / 2, (BlobPtr)wp + (int64_t)(2 * blockIdx.y) * (Kp / 2) * 64, acc);
#pragma unroll
    for (int mt = 0; mt < 2; mt++)
#pragma unroll
        for (int nt = 0; nt < 2; nt++)
#pragma unroll
            for (int v = 0; v < 16; v++) {
                const int64_t r = row0 + 32 * mt + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3);
                const int c = 64 * blockIdx.y + 32 * nt + (lane & 31);
                if (r < M && c < N) y[r * N + c] = acc[mt][nt][v];
            }
}

// ---- bf16 precision: k_pol_trunk_bf16 ---------------------------------------
//
// DESIGN.md §2 definition 17: dense inputs and weights rounded to bf16, exact
// products, f32 accumulation in the order v_mfma_f32_32x32x16_bf16 takes,
// LayerNorm over the unrounded f32 outputs.  The selection, the embed kernel,
// the tile records and the sampling are the f32 path's; the tile's
// activations are bf16 in LDS and the outputs stay in the accumulators until
// they are normalised, so a block asks for half the LDS and two share a CU.

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef const __attribute__((address_space(1))) bf16x8 *FragPtr; // the packed weights, a lane's 16 bytes at a time

constexpr int kLdb = 520;       // LDS row stride in bf16: 65 x 16 B, so the 16 lanes that ds_read_b128 serves
                                // together (rows r, r + 1, ..) start at 16 different 16-B slots of the 256-B bank row
constexpr int kLgStride = 65;   // the f32 logits over the activations, one row per lane
constexpr size_t kActBytes = (size_t)kTileRows * kLdb * sizeof(uint16_t);
constexpr size_t kTrunkLdsBf16 = kActBytes + (size_t)(8 * kTileRows + 2 * kTileRows) * sizeof(float);
static_assert(kTrunkLdsBf16 <= 80 * 1024, "two blocks of k_pol_trunk_bf16 per CU (160 KiB of LDS)");
static_assert((size_t)kTileRows * kLgStride * sizeof(float) <= kActBytes, "the logits fit over the activations");

__device__ __forceinline__ uint16_t toBf16(float f) { return __builtin_bit_cast(uint16_t, (__bf16)f); } // RNE

// acc[mt][nt] = X[row0 + 32 mt ..][0 .. 16 ksteps) . W[.., tile nt], X bf16 in
// LDS (row stride kLdb), W packed (policy.h packBf16) with wp at the first
// tile.  Lane l feeds A[l & 31][8 (l >> 5) + j] and B[8 (l >> 5) + j][l & 31].
template <int MT, int NT>
__device__ __forceinline__ void mfmaDenseBf16(const uint16_t *xs, int row0, int ksteps, FragPtr wp, f32x16 (&acc)[MT][NT])
{
    const int lane = threadIdx.x & 63;
    const uint16_t *xa = xs + (row0 + (lane & 31)) * kLdb + 8 * (lane >> 5);
    const FragPtr wb = wp + lane;
    const int64_t tileStride = (int64_t)ksteps * 64;
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
#pragma unroll
            for (int v = 0; v < 16; v++) acc[mt][nt][v] = 0.f;
    bf16x8 b[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) b[nt] = wb[nt * tileStride];
    for (int s = 0; s < ksteps; s++) {
        // the next step's weights are in flight while this step's MFMAs run (the last step loads itself again)
        const int sn = s + 1 < ksteps ? s + 1 : s;
        bf16x8 bn[NT], a[MT];
#pragma unroll
        for (int nt = 0; nt < NT; nt++) bn[nt] = wb[nt * tileStride + (int64_t)sn * 64];
#pragma unroll
        for (int mt = 0; mt < MT; mt++) a[mt] = *reinterpret_cast<const bf16x8 *>(xa + mt * 32 * kLdb + 16 * s);
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int nt = 0; nt < NT; nt++)
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
#pragma unroll
        for (int nt = 0; nt < NT; nt++) b[nt] = bn[nt];
    }
}

// the row of accumulator register v of tile mt in a lane of half h (the C/D map above storeTiles)
__device__ __forceinline__ int accRow(int mt, int v, int h) { return 32 * mt + 8 * (v >> 2) + 4 * h + (v & 3); }

// v + the v of the lane that the DPP control names (0xb1: lane ^ 1, 0x4e: lane ^ 2 in a quad;
// 0x141, 0x140: the mirror image in the lane's 8 and 16)
template <int kCtrl>
__device__ __forceinline__ float addDpp(float v)
{
    return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), kCtrl, 0xf, 0xf, false));
}

// the sum of v over the 32 lanes of the lane's half, in every one of them
__device__ __forceinline__ float halfSum(float v)
{
    v = addDpp<0xb1>(v);
    v = addDpp<0x4e>(v);
    v = addDpp<0x141>(v);
    v = addDpp<0x140>(v);
    return v + __shfl_xor(v, 16);
}

// The sum over a row's 512 outputs of f(acc), for all 64 rows: the lane's two
// column tiles, the 32 lanes of a half, then the eight waves through `part`
// (lane l of a wave writes the row of register l & 15 of row tile (l >> 4) & 1).
// fin(sum) of row tid goes to out[tid]; the block has passed a barrier when
// this returns.
template <typename F, typename G>
__device__ __forceinline__ void rowStat(const f32x16 (&acc)[2][2], float *part, float *out, F f, G fin)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float mine = 0.f;
#pragma unroll
    for (int mt = 0; mt < 2; mt++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float sum = halfSum(f(acc[mt][0][r]) + f(acc[mt][1][r]));
            if ((lane & 31) == 16 * mt + r) mine = sum;
        }
    part[wave * kTileRows + accRow((lane >> 4) & 1, lane & 15, lane >> 5)] = mine;
    __syncthreads();
    if (tid < kTileRows) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < 8; w++) t += part[w * kTileRows + tid];
        out[tid] = fin(t);
    }
    __syncthreads();
}

// Same grid, tile records, fwdSlot convention and outputs as k_pol_trunk.
__global__ void __launch_bounds__(kTrunkThreads, 4) k_pol_trunk_bf16(DevState S, PolicyDev P, Layout L, LayoutBf16 B,
                                                                     int fwdSlot, float *logitsOut, int32_t *actionsOut)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    uint16_t *xs = reinterpret_cast<uint16_t *>(lds);    // [64][kLdb] activations, bf16
    float *part = lds + kActBytes / sizeof(float);       // [8 waves][64 rows] partial row sums
    float *mean = part + 8 * kTileRows, *sigma = mean + kTileRows;
    float *lgs = lds;                                    // [64][kLgStride] logits, once the heads have read xs

    const bool useList = fwdSlot < 0;
    const int64_t base = (int64_t)blockIdx.x * kTileRows;
    int64_t n = S.A; // one past the tile's last live row
    BlobPtr blob;
    if (useList) {
        const Tile t = P.tiles[blockIdx.x];
        blob = (BlobPtr)t.blob;
        n = base + t.rows;
    } else {
        blob = (BlobPtr)P.blobs[fwdSlot];
    }
    if (base >= n) return; // past the list
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = lane >> 5;

    for (int idx = tid; idx < kTileRows * (kTrunkIn / 2); idx += kTrunkThreads) { // the f32 trunk inputs, two at a time
        const int r = idx / (kTrunkIn / 2), c = 2 * (idx - r * (kTrunkIn / 2));
        float2 x = make_float2(0.f, 0.f);
        if (base + r < n) x = *reinterpret_cast<const float2 *>(P.emb + (base + r) * kTrunkIn + c);
        *reinterpret_cast<uint32_t *>(xs + r * kLdb + c) = (uint32_t)toBf16(x.x) | ((uint32_t)toBf16(x.y) << 16);
    }
    __syncthreads();

    for (int layer = 0; layer < 3; layer++) {
        const int ksteps = (layer == 0 ? kTrunkIn : kHidden) / 16;
        f32x16 acc[2][2];
        mfmaDenseBf16<2, 2>(xs, 0, ksteps, (FragPtr)(blob + B.trunkW[layer]) + (int64_t)(2 * wave) * ksteps * 64, acc);
        // mean, then the biased variance of the deviations, over the unrounded outputs
        rowStat(acc, part, mean, [](float y) { return y; }, [](float t) { return t * (1.f / (float)kHidden); });
#pragma unroll
        for (int mt = 0; mt < 2; mt++)
#pragma unroll
            for (int v = 0; v < 16; v++) {
                const float m = mean[accRow(mt, v, half)];
                acc[mt][0][v] -= m;
                acc[mt][1][v] -= m;
            }
        rowStat(acc, part, sigma, [](float d) { return d * d; },
                [](float t) { return mp::sqrt_(t / (float)kHidden + 1e-6f); });
        // every wave is past its MFMAs: the tile's inputs make way for its outputs
        const int col = 64 * wave + (lane & 31);
        const float sc[2] = { blob[L.trunkScale[layer] + col], blob[L.trunkScale[layer] + col + 32] };
        const float bs[2] = { blob[L.trunkBias[layer] + col], blob[L.trunkBias[layer] + col + 32] };
#pragma unroll
        for (int mt = 0; mt < 2; mt++)
#pragma unroll
            for (int v = 0; v < 16; v++) {
                const int r = accRow(mt, v, half);
                const float sg = sigma[r];
#pragma unroll
                for (int nt = 0; nt < 2; nt++) {
                    const float o = mp::fma_(sc[nt] / sg, acc[mt][nt][v], bs[nt]);
                    xs[r * kLdb + col + 32 * nt] = toBf16(o >= 0.f ? o : 0.f * o);
                }
            }
        __syncthreads();
    }

    // both heads as one 512 x 64 dense: four waves, one 32 x 32 tile each
    f32x16 hacc[1][1];
    const int mt = wave & 1, nt = (wave >> 1) & 1;
    if (wave < 4) mfmaDenseBf16<1, 1>(xs, 32 * mt, kHidden / 16, (FragPtr)(blob + B.headW) + (int64_t)nt * (kHidden / 16) * 64, hacc);
    __syncthreads();
    if (wave < 4)
#pragma unroll
        for (int v = 0; v < 16; v++) lgs[accRow(mt, v, half) * kLgStride + 32 * nt + (lane & 31)] = hacc[0][0][v];
    __syncthreads();

    // from here on as k_pol_trunk: bias, logits out, the six draws
    if (tid >= kTileRows || base + tid >= n) return;
    const int64_t g = useList ? (int64_t)P.list[base + tid] : base + tid;
    float *lg = lgs + tid * kLgStride; // the agent's own row
    for (int j = 0; j < kLogits; j++) lg[j] = lg[j] + blob[L.headBias + j];
    if (logitsOut)
        for (int j = 0; j < kLogits; j++) logitsOut[g * kLogits + j] = lg[j];
    if (!useList && !actionsOut) return;

    constexpr int kBuckets[kNumHeads] = { 3, 8, 3, 3, 13, 7 };
    mp::RNG rng;
    rng.key.a = (uint32_t)S.rngA[g];
    rng.key.b = (uint32_t)S.rngB[g];
    rng.ctr = (uint32_t)S.rngCtr[g];
    int32_t act[kNumHeads];
    int at = 0;
#pragma unroll
    for (int h = 0; h < kNumHeads; h++) {
        act[h] = sampleHead(lg + at, kBuckets[h], mp::rngAdvance(rng));
        at += kBuckets[h];
    }
    if (useList) {
        reinterpret_cast<int4 *>(S.discreteAction)[g] = make_int4(act[0], act[1], act[2], act[3]);
        reinterpret_cast<int2 *>(S.discreteAim)[g] = make_int2(act[4], act[5]);
        S.rngCtr[g] = (int32_t)rng.ctr;
    } else {
        for (int h = 0; h < kNumHeads; h++) actionsOut[g * kNumHeads + h] = act[h];
    }
}

// mpenv_debug_policy_dense_bf16: one wave per 64 x 64 output tile through mfmaDenseBf16
__global__ void __launch_bounds__(64) k_pol_dense_bf16(const float *x, int M, int K, const uint16_t *wp, int N, float *y)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    uint16_t *xs = reinterpret_cast<uint16_t *>(lds);
    const int lane = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kTileRows;
    const int Kp = (K + 15) & ~15;
    for (int idx = lane; idx < kTileRows * Kp; idx += 64) {
        const int r = idx / Kp, c = idx - r * Kp;
        xs[r * kLdb + c] = toBf16((row0 + r < M && c < K) ? x[(row0 + r) * K + c] : 0.f);
    }
    __syncthreads();
    f32x16 acc[2][2];
    mfmaDenseBf16<2, 2>(xs, 0, Kp / 16, (FragPtr)wp + (int64_t)(2 * blockIdx.y) * (Kp / 16) * 64, acc);
#pragma unroll
    for (int mt = 0; mt < 2; mt++)
#pragma unroll
        for (int nt = 0; nt < 2; nt++)
#pragma unroll
            for (int v = 0; v < 16; v++) {
                const int64_t r = row0 + accRow(mt, v, lane >> 5);
                const int c = 64 * blockIdx.y + 32 * nt + (lane & 31);
                if (r < M && c < N) y[r * N + c] = acc[mt][nt][v];
            }
}

int check(hipError_t e) { return e == hipSuccess ? 0 : -1; }

int run(const DevState &s, const PolicyDev &p, int fwdSlot, float *logits, int32_t *actions, hipStream_t st,
        int precision, int parts = kPolicyEmbed | kPolicyTrunk)
{
    const bool bf16 = precision == MPENV_POLICY_BF16;
    if (!bf16 && precision != MPENV_POLICY_F32) return -1;
    if (hipFuncSetAttribute(bf16 ? reinterpret_cast<const void *>(k_pol_trunk_bf16)
                                 : reinterpret_cast<const void *>(k_pol_trunk),
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(bf16 ? kTrunkLdsBf16 : kTrunkLds)) != hipSuccess)
        return -1;
    const Layout L = layout();
    const int64_t perBlock = kEmbedWaves * kEmbedAgents;
    const int64_t rows = fwdSlot < 0 ? listRows(s.A) : s.A; // blocks past the last segment leave at once
    if (parts & kPolicyEmbed)
        hipLaunchKernelGGL(k_pol_embed, dim3((unsigned)((rows + perBlock - 1) / perBlock)), dim3(kEmbedWaves * 64), 0,
                           st, s, p, L, fwdSlot);
    if (check(hipGetLastError())) return -1;
    if (!(parts & kPolicyTrunk)) return 0;
    const dim3 tiles((unsigned)((rows + kTileRows - 1) / kTileRows));
    if (bf16)
        hipLaunchKernelGGL(k_pol_trunk_bf16, tiles, dim3(kTrunkThreads), kTrunkLdsBf16, st, s, p, L, layoutBf16(),
                           fwdSlot, logits, actions);
    else
        hipLaunchKernelGGL(k_pol_trunk, tiles, dim3(kTrunkThreads), kTrunkLds, st, s, p, L, fwdSlot, logits, actions);
    return check(hipGetLastError());
}

} // namespace

int launchPolicyStep(const DevState &s, const PolicyDev &p, void *stream, int parts, int precision)
{
    hipStream_t st = (hipStream_t)stream;
    if (parts & kPolicySelect) {
        const dim3 grid((unsigned)((s.A + kSelThreads - 1) / kSelThreads));
        if (check(hipMemsetAsync(p.count, 0, kSlots * sizeof(int32_t), st))) return -1;
        hipLaunchKernelGGL(k_pol_count, grid, dim3(kSelThreads), 0, st, s, p);
        hipLaunchKernelGGL(k_pol_plan, dim3(1), dim3(64), 0, st, p, (int)listTiles(s.A));
        hipLaunchKernelGGL(k_pol_scatter, grid, dim3(kSelThreads), 0, st, s, p);
        if (check(hipGetLastError())) return -1;
    }
    return run(s, p, -1, nullptr, nullptr, st, precision, parts);
}

int launchPolicyForward(const DevState &s, const PolicyDev &p, int slot, float *logits, int32_t *actions, void *stream,
                        int precision)
{
    if (slot < 0 || slot >= kSlots || !((p.mask >> slot) & 1u)) return -1;
    return run(s, p, slot, logits, actions, (hipStream_t)stream, precision);
}

// wPacked: pol::packB of w with N padded to a multiple of 64 columns
int launchPolicyDense(const float *x, int M, int K, const float *wPacked, int N, float *y, void *stream)
{
    if (M < 1 || N < 1 || K < 1 || K > kHidden) return -1;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_pol_dense), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)kDenseLds) != hipSuccess)
        return -1;
    hipLaunchKernelGGL(k_pol_dense, dim3((unsigned)((M + kTileRows - 1) / kTileRows), (unsigned)((N + 63) / 64)),
                       dim3(64), kDenseLds, (hipStream_t)stream, x, M, K, wPacked, N, y);
    return check(hipGetLastError());
}

// wPacked: pol::packBf16 of w with N padded to a multiple of 64 columns
int launchPolicyDenseBf16(const float *x, int M, int K, const uint16_t *wPacked, int N, float *y, void *stream)
{
    if (M < 1 || N < 1 || K < 1 || K > kHidden) return -1;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_pol_dense_bf16), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)kActBytes) != hipSuccess)
        return -1;
    hipLaunchKernelGGL(k_pol_dense_bf16, dim3((unsigned)((M + kTileRows - 1) / kTileRows), (unsigned)((N + 63) / 64)),
                       dim3(64), kActBytes, (hipStream_t)stream, x, M, K, wPacked, N, y);
    return check(hipGetLastError());
}

} // namespace mpenv
