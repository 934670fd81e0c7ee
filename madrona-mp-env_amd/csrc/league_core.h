// league_core.h — the league scheduler's arithmetic (DESIGN.md §2 definition
// 20, include/mpenv_league.h), once for host and device: k_league
// (league.hip) and the host entry points mpenv_league_draw / _record
// (league.cpp) call these functions and nothing else decides a bucket, a team
// id, a pick, a draw value or what an episode adds to the standings.
#pragma once

#include "mpenv_core.h"

namespace mp {

constexpr int kLeagueMaxPolicies = 32; // MPENV_POLICY_SLOTS
constexpr int kLeagueCols = 8;         // episodes, wins 0, wins 1, draws, kills 0/1, zone points 0/1
constexpr uint32_t kLeagueKeyUpper = 0x4c454147u; // "LEAG"
constexpr int32_t kLeagueMaxWeight = 65535;

enum : int32_t { kLeagueDrawNone = 0, kLeagueDrawTeam1 = 1, kLeagueDrawBoth = 2 };

// null for a valid configuration, else the limit it misses
MP_HD const char *leagueConfigError(int32_t num_policies, int32_t draw)
{
    if (num_policies < 1 || num_policies > kLeagueMaxPolicies) return "num_policies must be in [1, 32]";
    if (draw < kLeagueDrawNone || draw > kLeagueDrawBoth)
        return "draw must be MPENV_LEAGUE_DRAW_NONE, MPENV_LEAGUE_DRAW_TEAM1 or MPENV_LEAGUE_DRAW_BOTH";
    return nullptr;
}

// bucket(p) = p for 0 <= p < P, else P: external (negative), out of range and mixed
MP_HD int leagueBucket(int32_t p, int P) { return p >= 0 && p < P ? (int)p : P; }

// The id of a team from its T AGENT_POLICY rows: the first agent's value
// when every agent holds it, else -1 (mixed)
MP_HD int32_t leagueTeamId(const int32_t *policy, int T)
{
    const int32_t first = policy[0];
    for (int k = 1; k < T; k++)
        if (policy[k] != first) return -1;
    return first;
}

MP_HD uint32_t leagueWeight(int32_t w) { return (uint32_t)(w < 0 ? 0 : (w > kLeagueMaxWeight ? kLeagueMaxWeight : w)); }

// pick(row, x): -1 (no change) for a row whose clamped sum is 0, else the
// smallest j whose inclusive prefix sum exceeds mulhi(x, sum)
MP_HD int32_t leaguePick(const int32_t *row, int P, uint32_t x)
{
    uint32_t tot = 0;
    for (int j = 0; j < P; j++) tot += leagueWeight(row[j]);
    if (tot == 0) return -1;
    const uint32_t r = (uint32_t)mulhi(x, tot); // tot <= 32 * 65535 < 2^31
    uint32_t acc = 0;
    for (int j = 0; j < P; j++) {
        acc += leagueWeight(row[j]);
        if (acc > r) return j;
    }
    return P - 1; // not reached: r < tot
}

// the draw value of world `global_world`'s n-th visit
MP_HD RandKey leagueDrawValue(uint32_t seed, uint32_t global_world, uint32_t n)
{
    return threefry2x32(initKey(seed, kLeagueKeyUpper), global_world, n);
}

// One visit's draw from the two team ids as they stand: ids[k] becomes the
// pick where team k is re-drawn and set[k] says so (its T rows are written).
// weights is [P + 1][P].
MP_HD void leagueDrawTeams(int32_t mode, int P, const int32_t *weights, RandKey h, int32_t ids[2], bool set[2])
{
    set[0] = set[1] = false;
    if (mode == kLeagueDrawNone) return;
    if (mode == kLeagueDrawBoth) {
        const int32_t p0 = leaguePick(weights + (size_t)P * P, P, h.a);
        if (p0 >= 0) {
            ids[0] = p0;
            set[0] = true;
        }
    }
    const int32_t p1 = leaguePick(weights + (size_t)leagueBucket(ids[0], P) * P, P, h.b);
    if (p1 >= 0) {
        ids[1] = p1;
        set[1] = true;
    }
}

// What one ended episode adds to its cell, from MATCH_RESULT's first five values
MP_HD void leagueAddends(const int32_t *mr, int32_t add[kLeagueCols])
{
    add[0] = 1;
    add[1] = mr[0] == 0;
    add[2] = mr[0] == 1;
    add[3] = mr[0] == 2;
    add[4] = mr[1];
    add[5] = mr[2];
    add[6] = mr[3];
    add[7] = mr[4];
}

// the cell of an episode between team ids i0 and i1, as an index of [P + 1][P + 1]
MP_HD int leagueCell(int32_t i0, int32_t i1, int P) { return leagueBucket(i0, P) * (P + 1) + leagueBucket(i1, P); }

} // namespace mp
