// curriculum.hip — k_harvest: the live curriculum pool (DESIGN.md §2
// definition 21): behind every step, each slot of the pool that refreshes at
// this tick and whose candidate world passes the filter takes that world's
// packed match state and players.  A kernel beside the step, launched behind
// it while a pool is enabled; the arithmetic is curriculum_core.h's.
#include "curriculum.h"
#include "curriculum_core.h"

namespace mpenv {

constexpr int kHarvestGroup = 16;                           // lanes per slot: 12 player lanes, a header lane, 3 idle
constexpr int kHarvestBlock = 64;                           // one wave
constexpr int kHarvestSlots = kHarvestBlock / kHarvestGroup; // slots per wave
constexpr int kSnapBytes = (int)sizeof(mpenv_curriculum_snapshot);
constexpr int kSnapQuads = kSnapBytes / 16;
static_assert(kSnapBytes == 176 && kSnapBytes % 16 == 0, "a snapshot is 11 16-B stores");
static_assert(mp::kCurriculumPlayers < kHarvestGroup && kSnapQuads <= kHarvestGroup, "a slot's lanes");
static_assert(sizeof(mpenv_packed_player) == 14 && offsetof(mpenv_curriculum_snapshot, players) == 8, "record layout");

// Slot-centric: lane group = slot, so no two lanes write one slot and nothing
// is atomic.  A block is one wave (its barrier is the wave's own, and the early
// exit is taken by the whole block): with period p a wave has a refreshing
// slot at about 4 / p of the ticks, and otherwise leaves after its range's
// two words, the hash and a ballot.  In a group, lane i < 12 packs player i and lane 12
// the match state into the slot's 176-B record in LDS; lanes 0..10 then store
// the record as 11 16-B vectors (the pool is 16-B aligned and 176 = 11 * 16).
// Only state columns are read, so the kernel is legal behind a direct
// gpuStreamStep, whose observation rows are elsewhere.
__global__ void __launch_bounds__(kHarvestBlock) k_harvest(DevState S, PoolDev P, uint32_t tick, int fill)
{
    __shared__ __attribute__((aligned(16))) unsigned char rec[kHarvestSlots][kSnapBytes];
    const int grp = (int)threadIdx.x / kHarvestGroup, l = (int)threadIdx.x % kHarvestGroup;
    const int64_t gs = (int64_t)blockIdx.x * kHarvestSlots + grp; // slot of [R][capacity], flat
    const bool valid = gs < (int64_t)P.R * P.capacity;
    const int r = valid ? (int)(gs / P.capacity) : 0;
    const int s = valid ? (int)(gs - (int64_t)r * P.capacity) : 0;
    const int first = P.ranges[2 * r], nw = P.ranges[2 * r + 1];
    int w = first + s % nw;
    bool refresh = valid;
    if (!fill)
        refresh = valid && mp::curriculumSelect(P.seed, P.worldOffset, (uint32_t)s, tick, (uint32_t)P.period, first, nw, &w);
    if (__ballot(refresh) == 0ull) return;

    const int N = S.N, T = S.T;
    const bool player = refresh && l < N; // N <= 12
    const int64_t g = (int64_t)w * N + (player ? l : 0);
    const float hp = player ? S.hp[g] : 0.f;
    // each team's living agents among the group's lanes
    const unsigned long long living = __ballot(player && hp > 0.f);
    const uint32_t mine = (uint32_t)(living >> (grp * kHarvestGroup)) & 0xffffu;
    const uint32_t team0 = (1u << T) - 1u;
    bool accept = refresh;
    if (refresh && !fill)
        accept = mp::curriculumAccept(S.finished[w], S.curStep[w], P.stepLo, P.stepHi, P.need, S.captured[w],
                                      S.contested[w], (mine & team0) != 0u, (mine & (team0 << T)) != 0u);

    if (accept && l < mp::kCurriculumPlayers) {
        mpenv_packed_player pl {};
        if (l < N)
            pl = mp::curriculumPackPlayer(S.px[g], S.py[g], S.pz[g], S.ayaw[g], S.apitch[g], hp, S.magazine[2 * g],
                                          S.magazine[2 * g + 1], S.curPose[g], S.landedOn[g]);
        uint16_t h[7];
        __builtin_memcpy(h, &pl, sizeof(pl));
        uint16_t *dst = reinterpret_cast<uint16_t *>(&rec[grp][8 + 14 * l]);
#pragma unroll
        for (int k = 0; k < 7; k++) dst[k] = h[k];
    } else if (accept && l == mp::kCurriculumPlayers) {
        mpenv_curriculum_snapshot head; // only the match state's 8 bytes are used
        mp::curriculumPackMatch(head, mp::curriculumLoggedStep(S.curStep[w]), S.curZone[w], S.captured[w],
                                S.controlling[w], S.zoneSteps[w], S.stepsUntilPoint[w]);
        uint16_t h[4];
        __builtin_memcpy(h, &head, sizeof(h));
        uint16_t *dst = reinterpret_cast<uint16_t *>(&rec[grp][0]);
#pragma unroll
        for (int k = 0; k < 4; k++) dst[k] = h[k];
        P.ticks[gs] = fill ? 0u : tick;
    }
    __syncthreads();
    if (accept && l < kSnapQuads)
        reinterpret_cast<uint4 *>(P.pool + gs)[l] = reinterpret_cast<const uint4 *>(&rec[grp][0])[l];
}

static int checkH(hipError_t e) { return e == hipSuccess ? 0 : -1; }

int launchHarvest(const DevState &s, const PoolDev &p, uint32_t tick, int fill, void *stream)
{
    if (s.W < 1 || !p.pool || !p.ticks || !p.ranges || p.R < 1 || p.capacity < 1) return -1;
    if (s.N < 1 || s.N > mp::kCurriculumPlayers) return -1;
    if (((uintptr_t)p.pool & 15u) != 0) return -1;
    const int64_t slots = (int64_t)p.R * p.capacity;
    const int64_t blocks = (slots + kHarvestSlots - 1) / kHarvestSlots;
    if (blocks > 0x7fffffffll) return -1;
    hipLaunchKernelGGL(k_harvest, dim3((unsigned)blocks), dim3(kHarvestBlock), 0, (hipStream_t)stream, s, p, tick, fill);
    return checkH(hipGetLastError());
}

} // namespace mpenv
