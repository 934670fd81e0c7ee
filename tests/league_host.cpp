// league_host.cpp — a stand-alone program over league_core.h's host functions,
// built by tests/test_league.py with -fsanitize=address,undefined and run
// directly: every array the functions index is exactly as large as the
// definition says (heap allocations, so a read or write past the end is seen),
// the weights span the whole int32 range, and the results are checked against
// a second, plainer statement of definition 20.  Prints "ok <checks>" and
// exits 0, or says what differed and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "league_core.h"

namespace {

uint64_t rngState = 0x9e3779b97f4a7c15ull;
uint32_t rnd()
{
    rngState = rngState * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rngState >> 32);
}

int64_t clampW(int64_t w) { return w < 0 ? 0 : (w > 65535 ? 65535 : w); }

// pick restated with 64-bit sums and a division-free search from the other end
int plainPick(const int32_t *row, int P, uint32_t x)
{
    int64_t tot = 0;
    for (int j = 0; j < P; j++) tot += clampW(row[j]);
    if (tot == 0) return -1;
    const int64_t r = (int64_t)(((unsigned __int128)x * (uint64_t)tot) >> 32);
    int best = -1;
    int64_t acc = tot;
    for (int j = P - 1; j >= 0; j--) { // the smallest j with prefix(j) > r
        if (acc > r) best = j;
        acc -= clampW(row[j]);
    }
    return best;
}

int fails = 0;
#define CHECK(cond, ...)                         \
    do {                                         \
        if (!(cond)) {                           \
            std::printf("FAILED: " __VA_ARGS__); \
            std::printf("\n");                   \
            fails++;                             \
        }                                        \
    } while (0)

} // namespace

int main()
{
    long checks = 0;
    const int32_t special[] = { 0, 1, -1, 65535, 65536, INT32_MAX, INT32_MIN, 7, 1000 };
    for (int iter = 0; iter < 4000; iter++) {
        const int P = iter % 4 == 0 ? 1 : (iter % 4 == 1 ? 32 : 1 + (int)(rnd() % 32));
        const int T = 1 + (int)(rnd() % 6);
        const int mode = (int)(rnd() % 3);
        std::vector<int32_t> weights((size_t)(P + 1) * P);
        const int kind = (int)(rnd() % 5);
        for (int32_t &v : weights) {
            switch (kind) {
            case 0: v = 0; break;
            case 1: v = (int32_t)(rnd() % 9 == 0 ? special[rnd() % 9] : 0); break;
            case 2: v = special[rnd() % 9]; break;
            case 3: v = (int32_t)rnd(); break;
            default: v = (int32_t)(rnd() % 100); break;
            }
        }
        std::vector<int32_t> ids((size_t)2 * T);
        for (int t = 0; t < 2; t++) {
            const int32_t id = (int32_t)(rnd() % (P + 4)) - 2;
            for (int k = 0; k < T; k++) ids[(size_t)t * T + k] = id;
            if (T > 1 && rnd() % 5 == 0) ids[(size_t)t * T + T - 1] = id + 1; // mixed
        }
        int32_t team[2] = { mp::leagueTeamId(ids.data(), T), mp::leagueTeamId(ids.data() + T, T) };
        for (int t = 0; t < 2; t++) {
            bool same = true;
            for (int k = 1; k < T; k++) same = same && ids[(size_t)t * T + k] == ids[(size_t)t * T];
            CHECK(team[t] == (same ? ids[(size_t)t * T] : -1), "team id, iter %d", iter);
            const int b = mp::leagueBucket(team[t], P);
            CHECK(b >= 0 && b <= P && (b == P || b == team[t]), "bucket, iter %d", iter);
        }
        const uint32_t seed = rnd(), world = rnd(), n = rnd() % 5;
        const mp::RandKey h = mp::leagueDrawValue(seed, world, n);
        const mp::RandKey h2 = mp::threefry2x32(mp::initKey(seed, 0x4c454147u), world, n);
        CHECK(h.a == h2.a && h.b == h2.b, "draw value, iter %d", iter);
        for (int r = 0; r <= P; r++) {
            const uint32_t x = r == 0 ? 0u : (r == 1 ? 0xffffffffu : rnd());
            const int got = mp::leaguePick(weights.data() + (size_t)r * P, P, x);
            CHECK(got == plainPick(weights.data() + (size_t)r * P, P, x), "pick, iter %d row %d", iter, r);
            CHECK(got >= -1 && got < P, "pick range, iter %d", iter);
            checks++;
        }
        int32_t now[2] = { team[0], team[1] };
        bool set[2];
        mp::leagueDrawTeams(mode, P, weights.data(), h, now, set);
        int32_t want[2] = { team[0], team[1] };
        if (mode == mp::kLeagueDrawBoth) {
            const int p0 = plainPick(weights.data() + (size_t)P * P, P, h.a);
            if (p0 >= 0) want[0] = p0;
        }
        if (mode != mp::kLeagueDrawNone) {
            const int p1 = plainPick(weights.data() + (size_t)mp::leagueBucket(want[0], P) * P, P, h.b);
            if (p1 >= 0) want[1] = p1;
        }
        CHECK(now[0] == want[0] && now[1] == want[1], "draw, iter %d mode %d", iter, mode);
        CHECK(mode == mp::kLeagueDrawBoth || !set[0], "team 0 written outside DRAW_BOTH, iter %d", iter);
        CHECK(mode != mp::kLeagueDrawNone || (!set[0] && !set[1]), "DRAW_NONE wrote, iter %d", iter);
        // one episode into a table of exactly (P + 1)^2 cells
        std::vector<int64_t> table((size_t)(P + 1) * (P + 1) * mp::kLeagueCols, 0);
        std::vector<int32_t> mr(5);
        mr[0] = (int32_t)(rnd() % 5) - 1;
        for (int k = 1; k < 5; k++) mr[k] = (int32_t)(rnd() % 50);
        int32_t add[mp::kLeagueCols];
        mp::leagueAddends(mr.data(), add);
        const int cell = mp::leagueCell(team[0], team[1], P);
        CHECK(cell >= 0 && cell < (P + 1) * (P + 1), "cell range, iter %d", iter);
        for (int k = 0; k < mp::kLeagueCols; k++) table[(size_t)cell * mp::kLeagueCols + k] += add[k];
        CHECK(add[0] == 1 && add[1] + add[2] + add[3] == (mr[0] >= 0 && mr[0] <= 2) && add[4] == mr[1] && add[7] == mr[4],
              "addends, iter %d", iter);
        checks += 4;
    }
    CHECK(mp::leagueConfigError(0, 0) && mp::leagueConfigError(33, 0) && mp::leagueConfigError(3, 3) &&
              mp::leagueConfigError(3, -1) && !mp::leagueConfigError(1, 0) && !mp::leagueConfigError(32, 2),
          "config limits");
    if (fails) return 1;
    std::printf("ok %ld\n", checks);
    return 0;
}
