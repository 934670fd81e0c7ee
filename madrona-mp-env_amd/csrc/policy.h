// policy.h — in-sim policy inference (DESIGN.md §2 definition 15): the fixed
// architecture of the reference's evalAgentPolicy (src/dnn.cpp:555-891), the
// layout of its parameters in one device blob, and the launchers.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "engine.h"

namespace mpenv {

namespace pol {

constexpr int kEmbed = 64;           // EMBED_SIZE (dnn.cpp:588)
constexpr int kPosFreqs = 8;         // NUM_POSITION_EMBEDDING_FREQUENCIES (dnn.cpp:589)
constexpr int kCoefs = 9;            // RewardHyperParams
constexpr int kSelfIn = kSelfObs + kCoefs + 3 * kPosFreqs * 2; // 100 (dnn.cpp:594-597)
constexpr int kFwdIn = kFwdRays * 4; // 256
constexpr int kRearIn = kRearRays * 4; // 64
constexpr int kTmSlots = 5, kOppSlots = 6;
constexpr int kTrunkIn = 6 * kEmbed; // 384
constexpr int kHidden = 512;         // MLP_BUFFER_SIZE (dnn.cpp:740)
constexpr int kDiscreteLogits = 17;  // 3 + 8 + 3 + 3 (dnn.cpp:155-160)
constexpr int kAimLogits = 20;       // 13 yaw + 7 pitch (consts.hpp discreteAimNum*Buckets)
constexpr int kLogits = kDiscreteLogits + kAimLogits; // 37
constexpr int kNumHeads = 6;         // moveAmount, moveAngle, fire, stand, yaw, pitch
constexpr int kHeadPad = 64;         // the two heads as one 512 x 37 dense, columns padded to two MFMA tiles

// Embed modules in blob order (the order evalAgentPolicy runs them).
enum Module { kModSelf = 0, kModFwd, kModRear, kModTm, kModOpp, kModLk, kNumModules };
constexpr int kModIn[kNumModules] = { kSelfIn, kFwdIn, kRearIn, kOtherObs, kOtherObs, kOtherObs };

// Normalisation parameters: means, then inverse sigmas, each in this order.
constexpr int kNormSelf = 0, kNormCoefs = kNormSelf + kSelfObs, kNormFwd = kNormCoefs + kCoefs,
              kNormRear = kNormFwd + 4, kNormTm = kNormRear + 4, kNormOpp = kNormTm + kOtherObs,
              kNormLk = kNormOpp + kOtherObs, kNormCount = kNormLk + kOtherObs; // 156

// MFMA B-operand packing of a [K][N] kernel (v_mfma_f32_32x32x2_f32: lane l
// holds B[k = l >> 5][j = l & 31]): column tile t (32 columns), k step s (two
// rows), lane l -> W[2 s + (l >> 5)][32 t + (l & 31)] at ((t * K/2 + s) * 64 + l).
// K is padded to even and N to a multiple of 32 with zeros (exact: a chain
// that starts at +0 never holds -0, so adding +0 * x changes nothing).
constexpr int64_t packedFloats(int K, int N) { return (int64_t)((N + 31) / 32) * ((K + 1) / 2) * 64; }

// The blob, in floats.
struct Layout {
    int64_t normMean, normInv;
    int64_t embedW[kNumModules];     // [K][64] as stored in the checkpoint ([in][out])
    int64_t embedScale[kNumModules], embedBias[kNumModules];
    int64_t trunkW[3];               // packed
    int64_t trunkScale[3], trunkBias[3];
    int64_t headW;                   // packed [512][37 -> 64]
    int64_t headBias;                // 37 (padded to 64)
    int64_t total;
};

inline Layout layout()
{
    Layout L {};
    int64_t o = 0;
    auto take = [&](int64_t n) { int64_t r = o; o += (n + 63) / 64 * 64; return r; }; // 256-B aligned pieces
    L.normMean = take(kNormCount);
    L.normInv = take(kNormCount);
    for (int m = 0; m < kNumModules; m++) {
        L.embedW[m] = take((int64_t)kModIn[m] * kEmbed);
        L.embedScale[m] = take(kEmbed);
        L.embedBias[m] = take(kEmbed);
    }
    for (int i = 0; i < 3; i++) {
        L.trunkW[i] = take(packedFloats(i == 0 ? kTrunkIn : kHidden, kHidden));
        L.trunkScale[i] = take(kHidden);
        L.trunkBias[i] = take(kHidden);
    }
    L.headW = take(packedFloats(kHidden, kHeadPad));
    L.headBias = take(kHeadPad);
    L.total = o;
    return L;
}

void packB(const float *w /*[K][N]*/, int K, int N, float *out /*packedFloats(K, N)*/);

// bf16 precision (DESIGN.md §2 definition 17).  B-operand packing of a [K][N]
// kernel for v_mfma_f32_32x32x16_bf16: column tile t (32 columns), k step s
// (16 rows), lane l with r = l & 31, h = l >> 5 holds W[16 s + 8 h + j][32 t + r],
// j = 0..7, as one 16-byte fragment at ((t * ceil(K/16) + s) * 64 + l) * 8 + j.
// K is padded to a multiple of 16 and N to a multiple of 32 with +0.
constexpr int64_t packedBf16(int K, int N) { return (int64_t)((N + 31) / 32) * ((K + 15) / 16) * 64 * 8; }
// f32 -> bf16, round to nearest even; a NaN stays a (quiet) NaN
inline uint16_t bf16Bits(float f)
{
    uint32_t u;
    __builtin_memcpy(&u, &f, sizeof(u));
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
void packBf16(const float *w /*[K][N]*/, int K, int N, uint16_t *out /*packedBf16(K, N)*/);

// The bf16 pieces of the blob, in floats, behind Layout::total: every blob
// carries both packings, and no offset of Layout moves.
struct LayoutBf16 {
    int64_t trunkW[3]; // packBf16
    int64_t headW;     // packBf16 [512][37 -> 64]
    int64_t total;     // the whole blob
};

inline LayoutBf16 layoutBf16()
{
    LayoutBf16 B {};
    int64_t o = layout().total;
    auto take = [&](int64_t halves) { int64_t r = o; o += (halves / 2 + 63) / 64 * 64; return r; };
    for (int i = 0; i < 3; i++) B.trunkW[i] = take(packedBf16(i == 0 ? kTrunkIn : kHidden, kHidden));
    B.headW = take(packedBf16(kHidden, kHeadPad));
    B.total = o;
    return B;
}

} // namespace pol

// policy.cpp: reads and validates a converted-checkpoint directory
// (loadPolicyWeights / loadNormParams, dnn.cpp:1066-1480); with `blob` also
// builds the device blob.  Returns MPENV_OK, MPENV_ERR_IO (a file that cannot
// be opened or is short) or MPENV_ERR_INVALID (rank / shape), `err` naming
// the file and the reason.
int policyRead(const char *dir, std::vector<float> *blob, std::string &err);

// policy.hip
//
// Checkpoint slots (MPENV_POLICY_SLOTS): an agent with policy id p >= 0 is
// served by slot p if 0 <= p < 32 and that slot holds a checkpoint, else by
// slot 0 if that holds one, else by nobody.  The selected agents are listed by
// slot, each slot's segment starting at a multiple of pol::kSegAlign list
// positions (one trunk tile, a multiple of the embed kernel's agents per
// block), so no embed wave and no trunk tile mixes checkpoints; the tail
// positions of a segment are dead (read as zeros, write nothing).
namespace pol {
constexpr int kSlots = 32;
constexpr int kSegAlign = 64;
// list positions / emb rows that hold any selection of A agents: the sum of
// the padded segments is a multiple of kSegAlign and at most A + 32 * 63
constexpr int64_t listTiles(int64_t A) { return (A + (int64_t)kSlots * (kSegAlign - 1)) / kSegAlign; }
constexpr int64_t listRows(int64_t A) { return listTiles(A) * kSegAlign; }
// one 64-row tile of the list: all an embed or trunk block needs, in one 16-B load
struct alignas(16) Tile {
    const float *blob;   // the checkpoint of the tile's slot
    int32_t rows;        // live rows: 64 but for a segment's last tile, 0 past the last segment
    int32_t slot;
};
// the allocation behind PolicyDev's counters and tiles: count[32], cursor[32], then the tiles
constexpr int64_t kTabHeadBytes = 2 * kSlots * sizeof(int32_t);
constexpr int64_t tabBytes(int64_t A) { return kTabHeadBytes + listTiles(A) * (int64_t)sizeof(Tile); }
} // namespace pol

struct PolicyDev {
    const float *const *blobs; // [32] device table: slot -> pol::layout() blob, null while empty
    uint32_t mask;       // bit s: slot s holds a checkpoint (the host's copy of blobs[s] != null)
    float *emb;          // [listRows(A)][384] trunk inputs of the selected agents, by list position
    int32_t *list;       // [listRows(A)] selected agent ids, by slot
    int32_t *count;      // [32] agents per slot (zeroed in front of every selection)
    int32_t *cursor;     // [32] next free list position of each segment
    pol::Tile *tiles;    // [listTiles(A)] every tile, the dead ones behind the last segment included
};
// The step path: select the agents a slot serves, write their action columns, advance their RNG by 6.
// parts: which of its kernels run (all in a step; mpenv_debug_policy_step times them apart --
// the trunk alone reuses the list and the embeddings of the last full call).
enum PolicyParts { kPolicySelect = 1, kPolicyEmbed = 2, kPolicyTrunk = 4, kPolicyAll = 7 };
// precision: MPENV_POLICY_F32 (k_pol_trunk) or MPENV_POLICY_BF16 (k_pol_trunk_bf16); the other kernels are shared
int launchPolicyStep(const DevState &s, const PolicyDev &p, void *stream, int parts = kPolicyAll,
                     int precision = MPENV_POLICY_F32);
// Every agent through the checkpoint of `slot`, no engine state written: logits [A][37], actions [A][6] (or null).
int launchPolicyForward(const DevState &s, const PolicyDev &p, int slot, float *logits, int32_t *actions, void *stream,
                        int precision = MPENV_POLICY_F32);
// y[M][N] = x[M][K] . w through the trunk's MFMA dense; wPacked = pol::packB(w) in device memory.
int launchPolicyDense(const float *x, int M, int K, const float *wPacked, int N, float *y, void *stream);
// the same through the bf16 trunk's dense; wPacked = pol::packBf16(w), N padded to a multiple of 64 columns
int launchPolicyDenseBf16(const float *x, int M, int K, const uint16_t *wPacked, int N, float *y, void *stream);

} // namespace mpenv
