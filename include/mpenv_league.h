/* mpenv_league.h -- the league scheduler: standings and matchmaking on the
 * device (DESIGN.md §2 definition 20, INTEGRATION.md "League scheduling").
 * Included by mpenv.h; callers include that.  An extension: the reference
 * keeps this bookkeeping in its JAX learner (scripts/jax_train.py eval_elo /
 * update_population).
 *
 * A league is enabled per manager with P = num_policies in 1..32
 * (MPENV_POLICY_SLOTS), a draw mode and a seed.  The manager must run with
 * auto_reset.  While enabled, one kernel (k_league) runs behind every step and
 * every init -- mpenv_step, mpenv_step_async, mpenv_gpu_stream_step,
 * mpenv_init, mpenv_gpu_stream_init -- on that call's stream.  The step
 * itself is unchanged: the same captured graph with the league on or off.
 *
 * Buckets and team ids.  bucket(p) = p for 0 <= p < P, else P: bucket P
 * collects externally driven teams (negative ids), ids >= P and mixed teams.
 * A team's id is its first agent's AGENT_POLICY value when all team_size
 * agents of the team hold that value, else -1 (mixed).  Team 0 is a world's
 * first team_size agents, team 1 the rest.
 *
 * Standings.  MPENV_LEAGUE_TABLE is int64 [P+1][P+1][8], zero after enable.
 * A world ends an episode in a step when the step leaves DONE == 1 for the
 * world's first agent (with auto_reset the world was also reset in that step;
 * its MATCH_RESULT row survives the reset until the next episode's first
 * step).  For each such world, with i0, i1 the two team ids as they stand
 * after the step and before any redraw and mr its MATCH_RESULT row, cell
 * [bucket(i0)][bucket(i1)] takes
 *   [0] episodes      1           [4] kills of team 0        mr[1]
 *   [1] wins team 0   mr[0] == 0  [5] kills of team 1        mr[2]
 *   [2] wins team 1   mr[0] == 1  [6] zone points of team 0  mr[3]
 *   [3] draws         mr[0] == 2  [7] zone points of team 1  mr[4]
 * (any other mr[0] counts in column 0 only).  An episode ended by
 * mpenv_trigger_reset is recorded like any other.  Integer sums: the table
 * does not depend on the order of the additions and is exactly reproducible.
 *
 * Matchmaking.  MPENV_LEAGUE_WEIGHTS is int32 [P+1][P] in device memory,
 * writable by the caller (or mpenv_league_set_weights), all 1 after enable;
 * the kernel reads each entry clamped to [0, 65535].  MPENV_LEAGUE_DRAWS is
 * uint32 [W], zero after enable.  A world that ends an episode draws after it
 * is recorded; after mpenv_init / mpenv_gpu_stream_init every world draws
 * and nothing is recorded.  The draw value of a visit is
 *   h = threefry2x32(initKey(seed, 0x4c454147), world_id_offset + w, draws[w])
 * (two 32-bit words h.a, h.b), and draws[w] goes up by one on every visit,
 * whether or not ids changed.  pick(row, x): tot = the clamped row sum; tot ==
 * 0 is no change; else r = (x * tot) >> 32 and the pick is the smallest j
 * whose inclusive prefix sum exceeds r.
 *   MPENV_LEAGUE_DRAW_NONE   ids stay; standings only; draws stays 0.
 *   MPENV_LEAGUE_DRAW_TEAM1  team 1 gets pick(row bucket(i0), h.b); team 0,
 *                            the home side, is never written (an external
 *                            learner sits at id -1 and uses row P).
 *   MPENV_LEAGUE_DRAW_BOTH   team 0 gets pick(row P, h.a), then team 1 gets
 *                            pick(row bucket(team 0's id after that), h.b).
 * A pick is written to all team_size AGENT_POLICY rows of the team.  The
 * engine's own RNG columns are never touched.  New ids take effect at the
 * next step's policy evaluation.  mpenv_gpu_stream_step copies the caller's
 * pbt.policy_assignments buffer into AGENT_POLICY in front of every step: a
 * caller that wants the league's draws to stand passes that buffer as null.
 *
 * Refused with MPENV_ERR_INVALID, the reason named, the manager left as it
 * was: num_policies outside 1..32; an unknown draw mode; a manager without
 * auto_reset (a finished world would report done every step); a draw mode
 * other than NONE under MPENV_SIMFLAG_SUB_ZONES (the id also picks the
 * sub-zone inside the reset, which has happened by the time the draw runs).
 *
 * The table, the weights and draws are no part of the state: not in
 * snapshots, not on the wire, not in the trainInterface, and no export id
 * names them.  After mpenv_state_load the ids are the snapshot's and draws
 * continues from where it was.  Each rank of a sharded run keeps its own
 * table; the caller adds them.
 *
 * mpenv_league_enable called again replaces the league (zero table, unit
 * weights, zero draws); call it between steps.  mpenv_league_tensor,
 * _clear and _set_weights while disabled are MPENV_ERR_INVALID.  The pointers
 * mpenv_league_tensor returns hold until the next enable or disable.
 *
 * Without a manager or a GPU: mpenv_league_layout gives the three buffers'
 * bytes; mpenv_league_draw performs visit n of global world `global_world` on
 * ids_inout [2][team_size] with weights [P+1][P] (null: all 1);
 * mpenv_league_record adds one ended episode to table_inout [P+1][P+1][8].
 * They are the code the kernel runs. */
#ifndef MPENV_LEAGUE_H
#define MPENV_LEAGUE_H

#include "mpenv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPENV_LEAGUE_DRAW_NONE 0
#define MPENV_LEAGUE_DRAW_TEAM1 1
#define MPENV_LEAGUE_DRAW_BOTH 2

#define MPENV_LEAGUE_TABLE 0
#define MPENV_LEAGUE_WEIGHTS 1
#define MPENV_LEAGUE_DRAWS 2

#define MPENV_LEAGUE_COLUMNS 8

typedef struct mpenv_league_config {
    int32_t num_policies;
    int32_t draw;
    uint32_t seed;
    int32_t reserved;
} mpenv_league_config;

int mpenv_league_enable(mpenv_manager *mgr, const mpenv_league_config *cfg);
int mpenv_league_disable(mpenv_manager *mgr);
int mpenv_league_enabled(mpenv_manager *mgr, mpenv_league_config *out /* may be null */, int32_t *on);
int mpenv_league_tensor(mpenv_manager *mgr, int32_t which, void **ptr, int32_t *dtype, int32_t *ndim, int64_t *dims,
                        int32_t *gpu_id);
/* zeroes the table on hip_stream (null: the manager's own); asynchronous */
int mpenv_league_clear(mpenv_manager *mgr, void *hip_stream);
/* host [P+1][P] -> the device weights, ordered on the manager's stream and waited for */
int mpenv_league_set_weights(mpenv_manager *mgr, const int32_t *host);
int mpenv_league_layout(const mpenv_league_config *cfg, uint32_t num_worlds, int64_t *table_bytes,
                        int64_t *weights_bytes, int64_t *draws_bytes);
int mpenv_league_draw(const mpenv_league_config *cfg, uint32_t global_world, uint32_t n, const int32_t *weights,
                      int32_t team_size, int32_t *ids_inout);
int mpenv_league_record(const mpenv_league_config *cfg, const int32_t *match_result5, const int32_t *ids,
                        int32_t team_size, int64_t *table_inout);

#ifdef __cplusplus
}
#endif

#endif /* MPENV_LEAGUE_H */
