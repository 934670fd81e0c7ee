// curriculum_core.h — the curriculum snapshot's arithmetic (DESIGN.md §2
// definition 21, include/mpenv_curriculum.h), once for host and device: what
// a world's match state and players pack to (the event log's writeSnapshotD in
// kernels.hip and the pool's k_harvest in curriculum.hip run these lines, and
// so do the host entry points mpenv_curriculum_pool_pack / _select of
// curriculum.cpp), which slot of the pool refreshes at a tick, from which
// world, and whether that world passes the filter.
#pragma once

#include "mpenv.h"
#include "mpenv_core.h"

namespace mp {

constexpr int kCurriculumPlayers = 12;                  // mpenv_curriculum_snapshot::players
constexpr uint32_t kCurriculumKeyUpper = 0x43555252u;   // "CURR"
constexpr int32_t kPoseCrouch = 1, kPoseProne = 2;      // sim_dev.h kCrouch, kProne
enum : uint32_t { kNeedCaptured = 1u, kNeedContested = 2u, kNeedBothAlive = 4u, kNeedAll = 7u };

// One player's 14 bytes (writePackedStepSnapshot, sim.cpp:41-106): float ->
// i16 through i32 (in range except yaw == +pi, which wraps to -32768)
MP_HD mpenv_packed_player curriculumPackPlayer(float px, float py, float pz, float yaw, float pitch, float hp,
                                               int32_t mag, int32_t reloading, int32_t cur_pose, int32_t landed_on)
{
    mpenv_packed_player pl;
    pl.pos[0] = (int16_t)(int32_t)px;
    pl.pos[1] = (int16_t)(int32_t)py;
    pl.pos[2] = (int16_t)(int32_t)pz;
    pl.yaw = (int16_t)(int32_t)(yaw * 32768 / kPi);
    pl.pitch = (int16_t)(int32_t)(pitch * 32768 / kPi);
    pl.mag_num_bullets = (uint8_t)(uint16_t)mag;
    pl.is_reloading = (uint8_t)reloading;
    pl.hp = (uint8_t)hp;
    uint8_t fl = 0;
    if (landed_on != -1) fl |= 2;
    if (cur_pose == kPoseCrouch) fl |= 4;
    else if (cur_pose == kPoseProne) fl |= 8;
    pl.flags = fl;
    return pl;
}

// The match state's 8 bytes, into an mpenv_packed_step_snapshot or an
// mpenv_curriculum_snapshot (the same five members).  `step` is the value
// written: the step counter as it stood when the step began.
template <class Snap>
MP_HD void curriculumPackMatch(Snap &sn, int32_t step, int32_t cur_zone, int32_t captured, int32_t controlling,
                               int32_t zone_steps, int32_t steps_until_point)
{
    sn.step = (uint16_t)step;
    sn.cur_zone = (uint8_t)cur_zone;
    sn.cur_zone_controller = (int8_t)(captured ? controlling : -1);
    sn.zone_steps_remaining = (uint16_t)zone_steps;
    sn.steps_until_point = (uint16_t)steps_until_point;
}

// The step a record of a world between two steps carries: the event log
// writes its snapshot inside the step, before the step counter goes up, so
// the state a step leaves at curStep == c is logged under c - 1 (and the
// loader starts the episode at that value).  A world the step has just reset
// (c == 0) has no such record: 0.
MP_HD int32_t curriculumLoggedStep(int32_t cur_step) { return cur_step > 0 ? cur_step - 1 : 0; }

// The 64-bit value of slot `slot` at harvest tick `tick` of the range whose
// first world is global world `global_first` (world_id_offset + the range's
// first world in the batch): .a is the low word (does the slot refresh), .b
// the high word (from which world).  The range enters by that id alone, so
// range r of a map set draws what a single-map manager at that offset draws.
MP_HD RandKey curriculumSlotValue(uint32_t seed, uint32_t global_first, uint32_t slot, uint32_t tick)
{
    return threefry2x32(threefry2x32(initKey(seed, kCurriculumKeyUpper), global_first, 0u), slot, tick);
}

// Whether the slot refreshes at the tick, and the candidate world (an index
// of the batch: first_world + hi32 % num_worlds).  num_worlds >= 1.
MP_HD bool curriculumSelect(uint32_t seed, uint32_t world_id_offset, uint32_t slot, uint32_t tick, uint32_t period,
                            int32_t first_world, int32_t num_worlds, int32_t *world)
{
    const RandKey h = curriculumSlotValue(seed, world_id_offset + (uint32_t)first_world, slot, tick);
    *world = first_world + (int32_t)(h.b % (uint32_t)num_worlds);
    return period > 0 && h.a % period == 0;
}

// The filter a candidate world passes: not finished, its step inside the
// window, and every bit of `need`.  alive0 / alive1: the team has an agent
// with hp > 0.
MP_HD bool curriculumAccept(int32_t finished, int32_t cur_step, int32_t step_lo, int32_t step_hi, uint32_t need,
                            int32_t captured, int32_t contested, bool alive0, bool alive1)
{
    if (finished != 0 || cur_step < step_lo || cur_step > step_hi) return false;
    if ((need & kNeedCaptured) && !captured) return false;
    if ((need & kNeedContested) && !contested) return false;
    if ((need & kNeedBothAlive) && !(alive0 && alive1)) return false;
    return true;
}

// null for a valid configuration, else the limit it misses
MP_HD const char *curriculumConfigError(int32_t capacity, int32_t period, int32_t step_lo, int32_t step_hi, uint32_t need)
{
    if (capacity < 1) return "capacity must be >= 1";
    if (period < 0) return "period must be >= 0";
    if (step_lo > step_hi) return "step_lo must be <= step_hi";
    if (need & ~kNeedAll) return "need has bits other than MPENV_CURRICULUM_NEED_CAPTURED, _CONTESTED and _BOTH_ALIVE";
    return nullptr;
}

} // namespace mp
