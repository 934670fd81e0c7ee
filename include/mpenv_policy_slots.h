/* mpenv_policy_slots.h -- league play: one frozen checkpoint per policy id
 * inside the step.  Part of mpenv.h, which includes it; callers include
 * mpenv.h.  (DESIGN.md §2 definition 15.)
 *
 * A manager has MPENV_POLICY_SLOTS checkpoint slots, numbered from 0, each
 * empty or holding one checkpoint.  In every step an agent whose AGENT_POLICY
 * value is p
 *   p < 0                      keeps the actions it was given;
 *   0 <= p < 32, slot p holds  is evaluated by slot p's checkpoint;
 *   any other p >= 0           is evaluated by slot 0's checkpoint if slot 0
 *                              holds one; otherwise it is not evaluated: it
 *                              keeps its actions and its RNG does not move.
 * Everything else is per agent and the same for every slot: inputs,
 * normalisation, arithmetic, sampling, six RNG draws.  Under
 * MPENV_SIMFLAG_SUB_ZONES the same id also picks the agent's sub-zone, as
 * before.
 *
 * mpenv_policy_load_slot: mpenv_policy_load into the given slot (which is
 * mpenv_policy_load_slot(mgr, 0, dir)), with the same checks, refusals and
 * messages for every slot.  Loading into an occupied slot replaces that
 * slot's checkpoint between two steps (the league's hot swap) and leaves the
 * others alone; it waits for the manager's stream before the old parameters
 * are freed, and the captured step graph is not touched.  A load that fails
 * leaves the slot as it was.  MPENV_ERR_INVALID, the range named, for a slot
 * outside [0, MPENV_POLICY_SLOTS).
 * mpenv_policy_unload_slot empties one slot (no error if it is empty
 * already); it synchronises the device.  mpenv_policy_unload empties all of
 * them, and mpenv_policy_loaded says whether any holds a checkpoint.
 * mpenv_policy_slots: bit s of *mask is set while slot s holds a checkpoint.
 *
 * mpenv_policy_forward_slot: mpenv_policy_forward through the checkpoint of
 * the given slot for every agent, whatever its policy id (mpenv_policy_forward
 * is slot 0).  MPENV_ERR_INVALID for a slot out of range or empty. */
#ifndef MPENV_POLICY_SLOTS_H
#define MPENV_POLICY_SLOTS_H

#include "mpenv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPENV_POLICY_SLOTS 32

int mpenv_policy_load_slot(mpenv_manager *mgr, int32_t slot, const char *dir);
int mpenv_policy_unload_slot(mpenv_manager *mgr, int32_t slot);
int mpenv_policy_slots(mpenv_manager *mgr, uint32_t *mask);
int mpenv_policy_forward_slot(mpenv_manager *mgr, int32_t slot, float *logits_out_device,
                              int32_t *actions_out_device, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* MPENV_POLICY_SLOTS_H */
