/* mpenv_curriculum.h -- the live curriculum pool: episode starts harvested on
 * the device (DESIGN.md §2 definition 21, INTEGRATION.md "Live curriculum").
 * Included by mpenv.h; callers include that.  An extension: the reference
 * builds its curriculum file offline from an event log
 * (build_trajectory_curriculum.cpp).
 *
 * The engine starts half the episodes (not in eval mode) from one
 * mpenv_curriculum_snapshot of a table in device memory (level_gen.cpp:498-580).
 * Without a pool that table is the curriculum_data_path file given at
 * creation, or none.  mpenv_curriculum_pool_enable replaces it by a pool of
 * [R][capacity] snapshots, R the number of map ranges (1 for a single map):
 * the worlds of range r draw from row r, so a world only ever starts from a
 * state of its own map.  The reset code is unchanged and reads the pool in
 * place; the pool is always full (numSnapshots == capacity).
 *
 * Packing.  pack(w) is the 176 bytes the event log's
 * mpenv_packed_step_snapshot holds at bytes 16..191 for the state a step left
 * in world w: step = curStep - 1 (the event log writes inside the step,
 * before the counter goes up; 0 for a world the step has just reset), cur_zone,
 * cur_zone_controller = captured ? controlling : -1, zone_steps_remaining,
 * steps_until_point, then per player int16 positions (float -> int32 ->
 * int16), yaw and pitch * 32768 / pi the same way (yaw == +pi wraps to
 * -32768), magazine, reloading, hp (truncated to u8) and flags 2 (landedOn !=
 * -1), 4 (crouch), 8 (prone).  Players >= 2 * team_size are zero.
 *
 * Initial fill.  Enable fills slot s of range r with pack(first_world(r) + s %
 * num_worlds(r)), unfiltered, and sets its tick to 0.
 *
 * Harvest.  While enabled, one kernel (k_harvest) runs behind every step --
 * mpenv_step, mpenv_step_async, mpenv_gpu_stream_step (direct or copying) --
 * on that call's stream, outside the captured step graph; not behind an init.
 * Every step advances the tick t by one (the first step after enable is tick
 * 1).  For slot s of range r, with g = world_id_offset + first_world(r) the global
 * id of the range's first world,
 *   h = threefry2x32(threefry2x32(initKey(seed, 0x43555252), g, 0), s, t)
 * (the range enters through g alone: range r of a map set draws what a
 * single-map manager created at that offset draws); the slot refreshes when period > 0 and h.a % period == 0; its candidate is
 * world first_world(r) + h.b % num_worlds(r).  The candidate is accepted when
 * finished == 0, step_lo <= curStep <= step_hi and every bit of `need` holds
 * (CAPTURED: captured != 0; CONTESTED: contested != 0; BOTH_ALIVE: each team
 * has an agent with hp > 0), all read from the state the step left.  An
 * accepted slot becomes pack(candidate) and its tick t; any other slot keeps
 * its bytes and its tick.  Selection is by slot, so no two lanes write one
 * slot and the pool is exactly reproducible from (seed, world_id_offset).
 * period 0 harvests nothing; the tick still advances and the pool stays in
 * use.
 *
 * MPENV_CURRICULUM_POOL is uint8 [R][capacity][176], MPENV_CURRICULUM_TICKS
 * uint32 [R][capacity]: the tick of each slot's last write, 0 for the initial
 * fill or mpenv_curriculum_pool_set.  Both are device memory, 16-B aligned,
 * valid until the next enable or disable.  The bytes of a row are a
 * curriculum_data_path file.
 *
 * mpenv_curriculum_pool_enable needs a manager that has been initialised
 * (mpenv_init or mpenv_gpu_stream_init).  Refused with MPENV_ERR_INVALID, the
 * reason named, the manager left as it was: before an init; capacity < 1;
 * period < 0; step_lo > step_hi; unknown need bits; a manager opened with
 * replay_log_path.  Allowed with event_log_path, record_log_path, loaded
 * policies, a league, a camera, world groups and map sets.  Enable and disable
 * change the step kernels' arguments, so the step graph is re-captured once by
 * the next step; harvests never re-capture it.  Enable while enabled replaces
 * the pool.  Disable restores what creation set (the curriculum_data_path
 * table, or none) and frees the pool: a manager that never enabled a pool, or
 * has disabled it, steps exactly as before.
 *
 * mpenv_curriculum_pool_set writes n host snapshots into slots [first_slot,
 * first_slot + n) of a range, ordered on the manager's stream and waited for;
 * their ticks become 0.  A snapshot naming a zone the range's scene does not
 * have, or a controller outside [-1, 1], is refused as the file loader
 * refuses it.  mpenv_curriculum_pool_configure changes period, window, need
 * and seed (capacity must be the enabled one) without reallocating.
 *
 * Checkpoints.  The pool, its ticks and the tick counter are no part of the
 * state: not in snapshots, not on the wire, no export id.  After
 * mpenv_state_load the pool and the tick go on from where they were.
 *
 * Team sides.  Under MPENV_SIMFLAG_RANDOM_FLIP_TEAMS the format records no
 * side: see DESIGN.md §2 definition 21 for what a write followed by a read
 * does to each team.
 *
 * Without a manager or a GPU: mpenv_curriculum_pool_layout gives the two
 * buffers' bytes; mpenv_curriculum_pool_select says whether a slot refreshes
 * and names its candidate (`range` is the pool's row, below
 * MPENV_MAX_MAP_RANGES; the value depends on it through first_world only); mpenv_curriculum_pool_pack packs one world from
 * plain arrays.  They are the code the kernel runs. */
#ifndef MPENV_CURRICULUM_H
#define MPENV_CURRICULUM_H

#include "mpenv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPENV_CURRICULUM_NEED_CAPTURED 1u
#define MPENV_CURRICULUM_NEED_CONTESTED 2u
#define MPENV_CURRICULUM_NEED_BOTH_ALIVE 4u

#define MPENV_CURRICULUM_POOL 0
#define MPENV_CURRICULUM_TICKS 1

#define MPENV_CURRICULUM_SNAPSHOT_BYTES 176

typedef struct mpenv_curriculum_pool_config {
    int32_t capacity;         /* slots per map range, >= 1 */
    int32_t period;           /* a slot refreshes at a tick with probability 1 / period; 0: never */
    int32_t step_lo, step_hi; /* the window of curStep a candidate must be in (inclusive) */
    uint32_t need;            /* MPENV_CURRICULUM_NEED_* bits */
    uint32_t seed;
} mpenv_curriculum_pool_config;

/* One world's state as plain arrays, n = 2 * team_size agents each */
typedef struct mpenv_curriculum_world {
    int32_t cur_step, cur_zone, captured, controlling, zone_steps, steps_until_point;
    const float *pos;         /* [n][3] */
    const float *yaw, *pitch; /* [n] */
    const float *hp;          /* [n] */
    const int32_t *magazine;  /* [n][2]: bullets, reloading */
    const int32_t *cur_pose;  /* [n]: 0 stand, 1 crouch, 2 prone */
    const int32_t *landed_on; /* [n]: -1 none */
} mpenv_curriculum_world;

int mpenv_curriculum_pool_enable(mpenv_manager *mgr, const mpenv_curriculum_pool_config *cfg);
int mpenv_curriculum_pool_disable(mpenv_manager *mgr);
int mpenv_curriculum_pool_enabled(mpenv_manager *mgr, mpenv_curriculum_pool_config *out /* may be null */, int32_t *on);
int mpenv_curriculum_pool_tensor(mpenv_manager *mgr, int32_t which, void **ptr, int32_t *dtype, int32_t *ndim,
                                 int64_t *dims, int32_t *gpu_id);
/* how many harvest ticks have passed since enable */
int mpenv_curriculum_pool_tick(mpenv_manager *mgr, uint32_t *tick);
int mpenv_curriculum_pool_set(mpenv_manager *mgr, int32_t range, int32_t first_slot, int32_t n,
                              const mpenv_curriculum_snapshot *host);
int mpenv_curriculum_pool_configure(mpenv_manager *mgr, const mpenv_curriculum_pool_config *cfg);

int mpenv_curriculum_pool_layout(const mpenv_curriculum_pool_config *cfg, int32_t num_ranges, int64_t *pool_bytes,
                                 int64_t *ticks_bytes);
int mpenv_curriculum_pool_select(uint32_t seed, uint32_t world_id_offset, uint32_t range, uint32_t slot, uint32_t tick,
                                 int32_t period, int32_t first_world, int32_t num_worlds, int32_t *refresh,
                                 int32_t *world);
/* the record of a world between two steps (step = cur_step - 1, or 0) */
int mpenv_curriculum_pool_pack(const mpenv_curriculum_world *world, int32_t team_size, mpenv_curriculum_snapshot *out);

#ifdef __cplusplus
}
#endif

#endif /* MPENV_CURRICULUM_H */
