// league.hip — k_league: the league scheduler (DESIGN.md §2 definition 20):
// for every world that ended an episode in the step, the standings' cell of
// its two team ids takes the episode's result, and the world's teams are
// re-drawn from the weight rows.  A kernel beside the step, launched behind it
// while a league is enabled; the arithmetic is league_core.h's.
#include "league.h"
#include "league_core.h"

namespace mpenv {

constexpr int kLeagueBlock = 256;

// the sum of v over the wave's 64 lanes, in every lane
__device__ __forceinline__ long long waveSum(long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// Lane = world.  Almost every wave of almost every step has no finishing
// world and leaves after one load and a ballot.  In a wave that has some, the
// lanes that share a standings cell are summed first: the loop takes the
// distinct cells among the finishing lanes one at a time (the lowest such
// lane leads, its cell is broadcast), reduces the eight addends over the
// matching lanes, and the leader adds each non-zero column with one 64-bit
// device-scope atomic -- after a mass reset that is 8 atomics per (wave, cell)
// instead of 8 per world.  Integer sums: the table does not depend on order.
__global__ void __launch_bounds__(kLeagueBlock) k_league(DevState S, LeagueDev L, int initOnly)
{
    const int w = (int)(blockIdx.x * kLeagueBlock + threadIdx.x);
    const int lane = (int)(threadIdx.x & 63u);
    const int N = S.N, T = S.T, P = L.P;
    const bool fin = w < S.W && (initOnly || S.done[(int64_t)w * N] == 1);
    if (__ballot(fin) == 0ull) return;

    int32_t ids[2] = { -1, -1 };
    int32_t *pol = S.policy + (int64_t)(fin ? w : 0) * N;
    if (fin) {
        ids[0] = mp::leagueTeamId(pol, T);
        ids[1] = mp::leagueTeamId(pol + T, T);
    }

    if (!initOnly) {
        int32_t add[mp::kLeagueCols] = {};
        int cell = -1;
        if (fin) {
            mp::leagueAddends(S.matchResult + (int64_t)w * row::matchResult, add);
            cell = mp::leagueCell(ids[0], ids[1], P);
        }
        unsigned long long todo = __ballot(fin);
        while (todo) {
            const int leader = __ffsll(todo) - 1;
            const int c = __shfl(cell, leader, 64);
            const bool mine = fin && cell == c;
            todo &= ~__ballot(mine);
#pragma unroll
            for (int k = 0; k < mp::kLeagueCols; k++) {
                const long long sum = waveSum(mine ? (long long)add[k] : 0ll);
                if (lane == leader && sum != 0)
                    __hip_atomic_fetch_add(L.table + (int64_t)c * mp::kLeagueCols + k, sum, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }

    if (!fin || L.mode == mp::kLeagueDrawNone) return;
    const uint32_t n = L.draws[w];
    L.draws[w] = n + 1u;
    bool set[2];
    mp::leagueDrawTeams(L.mode, P, L.weights, mp::leagueDrawValue(L.seed, L.worldOffset + (uint32_t)w, n), ids, set);
    for (int t = 0; t < 2; t++)
        if (set[t])
            for (int k = 0; k < T; k++) pol[t * T + k] = ids[t];
}

static int checkL(hipError_t e) { return e == hipSuccess ? 0 : -1; }

int launchLeague(const DevState &s, const LeagueDev &lg, int initOnly, void *stream)
{
    if (s.W < 1 || !lg.table) return -1;
    const unsigned blocks = (unsigned)((s.W + kLeagueBlock - 1) / kLeagueBlock);
    hipLaunchKernelGGL(k_league, dim3(blocks), dim3(kLeagueBlock), 0, (hipStream_t)stream, s, lg, initOnly);
    return checkL(hipGetLastError());
}

} // namespace mpenv
