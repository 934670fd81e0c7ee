// curriculum.cpp — the live curriculum pool's entry points
// (include/mpenv_curriculum.h): configuration, the pool and its ticks, where the
// step kernels' SceneDev points, the launch behind every step, and the host
// restatement of a selection and of a packed world (curriculum_core.h).
#include <cstring>

#include "manager.h"

#include "curriculum_core.h"

namespace {

int badConfig(const mpenv_curriculum_pool_config *cfg)
{
    if (!cfg) return fail(MPENV_ERR_INVALID, "null argument");
    if (const char *why = mp::curriculumConfigError(cfg->capacity, cfg->period, cfg->step_lo, cfg->step_hi, cfg->need))
        return fail(MPENV_ERR_INVALID, why);
    return MPENV_OK;
}

int disabled(const char *who)
{
    return fail(MPENV_ERR_INVALID, std::string(who) + ": the curriculum pool is disabled (mpenv_curriculum_pool_enable first)");
}

// bytes of the pool and of the ticks; the pool's is a multiple of 16
struct Layout {
    size_t pool, ticks;
};

Layout layoutOf(int64_t R, int64_t capacity)
{
    return { (size_t)(R * capacity) * sizeof(mpenv_curriculum_snapshot), (size_t)(R * capacity) * sizeof(uint32_t) };
}

void applyConfig(PoolDev &p, const mpenv_curriculum_pool_config &c)
{
    p.period = c.period;
    p.stepLo = c.step_lo;
    p.stepHi = c.step_hi;
    p.need = c.need;
    p.seed = c.seed;
}

// Every range's (and world group's) step kernels read `table` + r * stride
// with n snapshots; table null: what creation set for the range's scene.
void pointScenes(mpenv_manager &m, const mpenv_curriculum_snapshot *table, int32_t n)
{
    for (size_t r = 0; r < m.ranges.size(); r++) {
        MapRange &mr = m.ranges[r];
        const SceneDev &made = m.scenes[mr.scene].sc;
        mr.sc.curriculum = table ? table + (size_t)r * n : made.curriculum;
        mr.sc.numSnapshots = table ? n : made.numSnapshots;
    }
    for (MapRange &g : m.groupRanges) { // sub-ranges of ranges[0]
        g.sc.curriculum = m.ranges[0].sc.curriculum;
        g.sc.numSnapshots = m.ranges[0].sc.numSnapshots;
    }
}

} // namespace

void mpenv_manager::runHarvest(hipStream_t st)
{
    poolTick++;
    if (pool.period == 0) return; // nothing refreshes
    launched(launchHarvest(S, pool, poolTick, 0, st), "k_harvest launch failed");
}

extern "C" {

int mpenv_curriculum_pool_layout(const mpenv_curriculum_pool_config *cfg, int32_t num_ranges, int64_t *pool_bytes,
                                 int64_t *ticks_bytes)
{
    if (int rc = badConfig(cfg)) return rc;
    if (num_ranges < 1 || num_ranges > MPENV_MAX_MAP_RANGES)
        return fail(MPENV_ERR_INVALID, "num_ranges must be in [1, MPENV_MAX_MAP_RANGES]");
    const Layout lay = layoutOf(num_ranges, cfg->capacity);
    if (pool_bytes) *pool_bytes = (int64_t)lay.pool;
    if (ticks_bytes) *ticks_bytes = (int64_t)lay.ticks;
    return MPENV_OK;
}

int mpenv_curriculum_pool_select(uint32_t seed, uint32_t world_id_offset, uint32_t range, uint32_t slot, uint32_t tick,
                                 int32_t period, int32_t first_world, int32_t num_worlds, int32_t *refresh,
                                 int32_t *world)
{
    if (!refresh || !world) return fail(MPENV_ERR_INVALID, "null argument");
    if (period < 0) return fail(MPENV_ERR_INVALID, "period must be >= 0");
    if (first_world < 0 || num_worlds < 1) return fail(MPENV_ERR_INVALID, "first_world must be >= 0 and num_worlds >= 1");
    if (range >= MPENV_MAX_MAP_RANGES) return fail(MPENV_ERR_INVALID, "range must be below MPENV_MAX_MAP_RANGES");
    // `range` names the pool's row; the value takes the range by its first world's global id
    *refresh = mp::curriculumSelect(seed, world_id_offset, slot, tick, (uint32_t)period, first_world, num_worlds, world) ? 1 : 0;
    return MPENV_OK;
}

int mpenv_curriculum_pool_pack(const mpenv_curriculum_world *w, int32_t team_size, mpenv_curriculum_snapshot *out)
{
    if (!w || !out || !w->pos || !w->yaw || !w->pitch || !w->hp || !w->magazine || !w->cur_pose || !w->landed_on)
        return fail(MPENV_ERR_INVALID, "null argument");
    if (team_size < 1 || team_size > kMaxTeamSize) return fail(MPENV_ERR_INVALID, "team_size must be in [1, 6]");
    const int N = 2 * team_size;
    std::memset(out, 0, sizeof(*out));
    mp::curriculumPackMatch(*out, mp::curriculumLoggedStep(w->cur_step), w->cur_zone, w->captured, w->controlling,
                            w->zone_steps, w->steps_until_point);
    for (int i = 0; i < N; i++)
        out->players[i] = mp::curriculumPackPlayer(w->pos[3 * i], w->pos[3 * i + 1], w->pos[3 * i + 2], w->yaw[i],
                                                   w->pitch[i], w->hp[i], w->magazine[2 * i], w->magazine[2 * i + 1],
                                                   w->cur_pose[i], w->landed_on[i]);
    return MPENV_OK;
}

int mpenv_curriculum_pool_enable(mpenv_manager *m, const mpenv_curriculum_pool_config *cfg)
{
    if (!m) return fail(MPENV_ERR_INVALID, "null manager");
    if (int rc = badConfig(cfg)) return rc;
    if (!m->inited)
        return fail(MPENV_ERR_INVALID, "the curriculum pool is filled from the batch: mpenv_init or mpenv_gpu_stream_init first");
    if (m->replayFile)
        return fail(MPENV_ERR_INVALID, "a manager opened with replay_log_path replays recorded states: no episode starts "
                                       "from a pool");
    return guarded([&] {
        // built aside and swapped in whole: a failed allocation leaves the
        // previous pool, or none, in place
        const int32_t R = (int32_t)m->ranges.size(), cap = cfg->capacity;
        const Layout lay = layoutOf(R, cap);
        std::vector<int32_t> tab;
        for (const MapRange &r : m->ranges) {
            if (r.w0 < 0 || r.n < 1 || (int64_t)r.w0 + r.n > m->S.W) throw std::runtime_error("a map range outside the batch");
            tab.push_back(r.w0);
            tab.push_back(r.n);
        }
        DevPtr buf;
        try {
            buf = DevPtr::create(lay.pool + lay.ticks + tab.size() * sizeof(int32_t));
        } catch (...) {
            (void)hipGetLastError(); // the next launch's error check must not see this one
            throw;
        }
        char *base = static_cast<char *>(buf.get());
        m->upload(base + lay.pool + lay.ticks, tab.data(), tab.size() * sizeof(int32_t)); // waits: no step is in flight
        PoolDev p {};
        p.pool = reinterpret_cast<mpenv_curriculum_snapshot *>(base);
        p.ticks = reinterpret_cast<uint32_t *>(base + lay.pool);
        p.ranges = reinterpret_cast<const int32_t *>(base + lay.pool + lay.ticks);
        p.R = R;
        p.capacity = cap;
        p.worldOffset = m->cfg.world_id_offset;
        applyConfig(p, *cfg);
        // every slot at once, unfiltered, from the batch as it stands
        launched(launchHarvest(m->S, p, 0, 1, m->stream), "k_harvest launch failed");
        HIP_CHECK(hipStreamSynchronize(m->stream));
        m->pool = p;
        m->poolCfg = *cfg;
        m->poolBuf = std::move(buf); // the previous buffer goes with `buf`
        m->poolTick = 0;
        m->poolOn = true;
        pointScenes(*m, p.pool, cap); // the next step re-captures its graph (argKey)
    });
}

int mpenv_curriculum_pool_disable(mpenv_manager *m)
{
    if (!m) return fail(MPENV_ERR_INVALID, "null manager");
    return guarded([&] {
        HIP_CHECK(hipStreamSynchronize(m->stream));
        if (m->poolOn) pointScenes(*m, nullptr, 0);
        m->poolOn = false;
        m->pool = PoolDev {};
        m->poolTick = 0;
        m->poolBuf = DevPtr {};
    });
}

int mpenv_curriculum_pool_enabled(mpenv_manager *m, mpenv_curriculum_pool_config *out, int32_t *on)
{
    if (!m || !on) return fail(MPENV_ERR_INVALID, "null argument");
    *on = m->poolOn ? 1 : 0;
    if (out) *out = m->poolOn ? m->poolCfg : mpenv_curriculum_pool_config {};
    return MPENV_OK;
}

int mpenv_curriculum_pool_tensor(mpenv_manager *m, int32_t which, void **ptr, int32_t *dtype, int32_t *ndim,
                                 int64_t *dims, int32_t *gpu_id)
{
    if (!m || !ptr || !dtype || !ndim || !dims) return fail(MPENV_ERR_INVALID, "null argument");
    if (!m->poolOn) return disabled("mpenv_curriculum_pool_tensor");
    dims[0] = m->pool.R;
    dims[1] = m->pool.capacity;
    switch (which) {
    case MPENV_CURRICULUM_POOL:
        *ptr = m->pool.pool;
        *dtype = MPENV_DTYPE_UINT8;
        *ndim = 3;
        dims[2] = sizeof(mpenv_curriculum_snapshot);
        break;
    case MPENV_CURRICULUM_TICKS:
        *ptr = m->pool.ticks;
        *dtype = MPENV_DTYPE_UINT32;
        *ndim = 2;
        break;
    default:
        return fail(MPENV_ERR_INVALID, "curriculum tensor must be MPENV_CURRICULUM_POOL or MPENV_CURRICULUM_TICKS");
    }
    if (gpu_id) *gpu_id = m->gpu;
    return MPENV_OK;
}

int mpenv_curriculum_pool_tick(mpenv_manager *m, uint32_t *tick)
{
    if (!m || !tick) return fail(MPENV_ERR_INVALID, "null argument");
    if (!m->poolOn) return disabled("mpenv_curriculum_pool_tick");
    *tick = m->poolTick;
    return MPENV_OK;
}

int mpenv_curriculum_pool_set(mpenv_manager *m, int32_t range, int32_t first_slot, int32_t n,
                              const mpenv_curriculum_snapshot *host)
{
    if (!m || !host) return fail(MPENV_ERR_INVALID, "null argument");
    if (!m->poolOn) return disabled("mpenv_curriculum_pool_set");
    if (range < 0 || range >= m->pool.R) return fail(MPENV_ERR_INVALID, "mpenv_curriculum_pool_set: no such map range");
    if (first_slot < 0 || n < 1 || (int64_t)first_slot + n > m->pool.capacity)
        return fail(MPENV_ERR_INVALID, "mpenv_curriculum_pool_set: slots outside [0, capacity)");
    // the file loader's check (manager_scene.cpp), against this range's scene
    const size_t zones = m->scenes[m->ranges[range].scene].scene.zoneAABBs.size();
    for (int32_t k = 0; k < n; k++)
        if (host[k].cur_zone >= zones || host[k].cur_zone_controller < -1 || host[k].cur_zone_controller > 1)
            return fail(MPENV_ERR_INVALID, "curriculum snapshot names a zone or controller outside the scene");
    return guarded([&] {
        const size_t at = (size_t)range * m->pool.capacity + first_slot;
        HIP_CHECK(hipMemsetAsync(m->pool.ticks + at, 0, (size_t)n * sizeof(uint32_t), m->stream));
        m->upload(m->pool.pool + at, host, (size_t)n * sizeof(mpenv_curriculum_snapshot));
    });
}

int mpenv_curriculum_pool_configure(mpenv_manager *m, const mpenv_curriculum_pool_config *cfg)
{
    if (!m) return fail(MPENV_ERR_INVALID, "null manager");
    if (int rc = badConfig(cfg)) return rc;
    if (!m->poolOn) return disabled("mpenv_curriculum_pool_configure");
    if (cfg->capacity != m->pool.capacity)
        return fail(MPENV_ERR_INVALID, "mpenv_curriculum_pool_configure keeps the capacity (mpenv_curriculum_pool_enable "
                                       "allocates another)");
    // launch arguments only: the next harvest runs with them
    applyConfig(m->pool, *cfg);
    m->poolCfg = *cfg;
    return MPENV_OK;
}

} // extern "C"
