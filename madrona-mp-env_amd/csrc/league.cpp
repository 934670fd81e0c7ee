// league.cpp — the league scheduler's entry points (include/mpenv_league.h):
// configuration, the three buffers, the launch behind every step and init, and
// the host restatement of a draw and of a recorded episode (league_core.h).
#include <cstring>

#include "manager.h"

#include "league_core.h"

namespace {

int badConfig(const mpenv_league_config *cfg)
{
    if (!cfg) return fail(MPENV_ERR_INVALID, "null argument");
    if (const char *why = mp::leagueConfigError(cfg->num_policies, cfg->draw)) return fail(MPENV_ERR_INVALID, why);
    return MPENV_OK;
}

int disabled(const char *who)
{
    return fail(MPENV_ERR_INVALID, std::string(who) + ": the league is disabled (mpenv_league_enable first)");
}

int badTeam(int32_t team_size)
{
    if (team_size < 1 || team_size > kMaxTeamSize) return fail(MPENV_ERR_INVALID, "team_size must be in [1, 6]");
    return MPENV_OK;
}

// bytes of the three buffers, each a multiple of 8
struct Layout {
    size_t table, weights, draws;
};

Layout layoutOf(int P, int64_t W)
{
    const auto up8 = [](size_t b) { return (b + 7) & ~size_t(7); };
    return { (size_t)(P + 1) * (P + 1) * mp::kLeagueCols * sizeof(int64_t), up8((size_t)(P + 1) * P * sizeof(int32_t)),
             up8((size_t)W * sizeof(uint32_t)) };
}

} // namespace

void mpenv_manager::runLeague(hipStream_t st, bool initOnly)
{
    // behind an init nothing is recorded, and without a draw mode nothing is drawn
    if (initOnly && league.mode == mp::kLeagueDrawNone) return;
    launched(launchLeague(S, league, initOnly ? 1 : 0, st), "k_league launch failed");
}

extern "C" {

int mpenv_league_layout(const mpenv_league_config *cfg, uint32_t num_worlds, int64_t *table_bytes,
                        int64_t *weights_bytes, int64_t *draws_bytes)
{
    if (int rc = badConfig(cfg)) return rc;
    if (num_worlds == 0) return fail(MPENV_ERR_INVALID, "num_worlds must be >= 1");
    const int P = cfg->num_policies;
    if (table_bytes) *table_bytes = (int64_t)(P + 1) * (P + 1) * mp::kLeagueCols * 8;
    if (weights_bytes) *weights_bytes = (int64_t)(P + 1) * P * 4;
    if (draws_bytes) *draws_bytes = (int64_t)num_worlds * 4;
    return MPENV_OK;
}

int mpenv_league_draw(const mpenv_league_config *cfg, uint32_t global_world, uint32_t n, const int32_t *weights,
                      int32_t team_size, int32_t *ids_inout)
{
    if (int rc = badConfig(cfg)) return rc;
    if (int rc = badTeam(team_size)) return rc;
    if (!ids_inout) return fail(MPENV_ERR_INVALID, "null argument");
    const int P = cfg->num_policies, T = team_size;
    int32_t ones[(mp::kLeagueMaxPolicies + 1) * mp::kLeagueMaxPolicies];
    if (!weights) {
        for (int32_t &v : ones) v = 1;
        weights = ones;
    }
    int32_t ids[2] = { mp::leagueTeamId(ids_inout, T), mp::leagueTeamId(ids_inout + T, T) };
    bool set[2];
    mp::leagueDrawTeams(cfg->draw, P, weights, mp::leagueDrawValue(cfg->seed, global_world, n), ids, set);
    for (int t = 0; t < 2; t++)
        if (set[t])
            for (int k = 0; k < T; k++) ids_inout[t * T + k] = ids[t];
    return MPENV_OK;
}

int mpenv_league_record(const mpenv_league_config *cfg, const int32_t *match_result5, const int32_t *ids,
                        int32_t team_size, int64_t *table_inout)
{
    if (int rc = badConfig(cfg)) return rc;
    if (int rc = badTeam(team_size)) return rc;
    if (!match_result5 || !ids || !table_inout) return fail(MPENV_ERR_INVALID, "null argument");
    const int P = cfg->num_policies, T = team_size;
    int32_t add[mp::kLeagueCols];
    mp::leagueAddends(match_result5, add);
    int64_t *cell = table_inout +
                    (size_t)mp::leagueCell(mp::leagueTeamId(ids, T), mp::leagueTeamId(ids + T, T), P) * mp::kLeagueCols;
    for (int k = 0; k < mp::kLeagueCols; k++) cell[k] += add[k];
    return MPENV_OK;
}

int mpenv_league_enable(mpenv_manager *m, const mpenv_league_config *cfg)
{
    if (!m) return fail(MPENV_ERR_INVALID, "null manager");
    if (int rc = badConfig(cfg)) return rc;
    if (!m->cfg.auto_reset)
        return fail(MPENV_ERR_INVALID, "the league needs auto_reset: a finished world would report done every step");
    if (cfg->draw != MPENV_LEAGUE_DRAW_NONE && (m->cfg.sim_flags & MPENV_SIMFLAG_SUB_ZONES))
        return fail(MPENV_ERR_INVALID, "under MPENV_SIMFLAG_SUB_ZONES only MPENV_LEAGUE_DRAW_NONE: the policy id also "
                                       "picks the sub-zone inside the reset, which precedes the draw");
    return guarded([&] {
        // built aside and swapped in whole: a failed allocation leaves the
        // previous league, or none, in place
        const int P = cfg->num_policies;
        const Layout lay = layoutOf(P, m->S.W);
        DevPtr buf;
        try {
            buf = DevPtr::create(lay.table + lay.weights + lay.draws);
        } catch (...) {
            (void)hipGetLastError(); // the next launch's error check must not see this one
            throw;
        }
        char *base = static_cast<char *>(buf.get());
        std::vector<int32_t> ones((size_t)(P + 1) * P, 1);
        HIP_CHECK(hipMemsetAsync(base, 0, lay.table + lay.weights + lay.draws, m->stream));
        m->upload(base + lay.table, ones.data(), ones.size() * sizeof(int32_t)); // waits: no k_league of the old one is in flight
        LeagueDev lg {};
        lg.table = reinterpret_cast<long long *>(base);
        lg.weights = reinterpret_cast<const int32_t *>(base + lay.table);
        lg.draws = reinterpret_cast<uint32_t *>(base + lay.table + lay.weights);
        lg.P = P;
        lg.mode = cfg->draw;
        lg.seed = cfg->seed;
        lg.worldOffset = m->cfg.world_id_offset;
        m->league = lg;
        m->leagueCfg = *cfg;
        m->leagueCfg.reserved = 0;
        m->leagueBuf = std::move(buf); // the previous buffer goes with `buf`
        m->leagueOn = true;
    });
}

int mpenv_league_disable(mpenv_manager *m)
{
    if (!m) return fail(MPENV_ERR_INVALID, "null manager");
    return guarded([&] {
        HIP_CHECK(hipStreamSynchronize(m->stream));
        m->leagueOn = false;
        m->league = LeagueDev {};
        m->leagueBuf = DevPtr {};
    });
}

int mpenv_league_enabled(mpenv_manager *m, mpenv_league_config *out, int32_t *on)
{
    if (!m || !on) return fail(MPENV_ERR_INVALID, "null argument");
    *on = m->leagueOn ? 1 : 0;
    if (out) *out = m->leagueOn ? m->leagueCfg : mpenv_league_config {};
    return MPENV_OK;
}

int mpenv_league_tensor(mpenv_manager *m, int32_t which, void **ptr, int32_t *dtype, int32_t *ndim, int64_t *dims,
                        int32_t *gpu_id)
{
    if (!m || !ptr || !dtype || !ndim || !dims) return fail(MPENV_ERR_INVALID, "null argument");
    if (!m->leagueOn) return disabled("mpenv_league_tensor");
    const int P = m->league.P;
    switch (which) {
    case MPENV_LEAGUE_TABLE:
        *ptr = m->league.table;
        *dtype = MPENV_DTYPE_INT64;
        *ndim = 3;
        dims[0] = dims[1] = P + 1;
        dims[2] = mp::kLeagueCols;
        break;
    case MPENV_LEAGUE_WEIGHTS:
        *ptr = const_cast<int32_t *>(m->league.weights);
        *dtype = MPENV_DTYPE_INT32;
        *ndim = 2;
        dims[0] = P + 1;
        dims[1] = P;
        break;
    case MPENV_LEAGUE_DRAWS:
        *ptr = m->league.draws;
        *dtype = MPENV_DTYPE_UINT32;
        *ndim = 1;
        dims[0] = m->S.W;
        break;
    default:
        return fail(MPENV_ERR_INVALID, "league tensor must be MPENV_LEAGUE_TABLE, MPENV_LEAGUE_WEIGHTS or MPENV_LEAGUE_DRAWS");
    }
    if (gpu_id) *gpu_id = m->gpu;
    return MPENV_OK;
}

int mpenv_league_clear(mpenv_manager *m, void *stream)
{
    if (!m) return fail(MPENV_ERR_INVALID, "null manager");
    if (!m->leagueOn) return disabled("mpenv_league_clear");
    return guarded([&] {
        HIP_CHECK(hipMemsetAsync(m->league.table, 0, layoutOf(m->league.P, m->S.W).table, streamOf(m, stream)));
    });
}

int mpenv_league_set_weights(mpenv_manager *m, const int32_t *host)
{
    if (!m || !host) return fail(MPENV_ERR_INVALID, "null argument");
    if (!m->leagueOn) return disabled("mpenv_league_set_weights");
    return guarded([&] {
        const int P = m->league.P;
        m->upload(const_cast<int32_t *>(m->league.weights), host, (size_t)(P + 1) * P * sizeof(int32_t));
    });
}

} // extern "C"
