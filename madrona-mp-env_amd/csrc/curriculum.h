// curriculum.h — what curriculum.hip (k_harvest) and curriculum.cpp (the
// mpenv_curriculum_pool_* entry points) share: the kernel's view of an enabled
// pool and its launcher.
#pragma once

#include <hip/hip_runtime.h>

#include "engine.h"

namespace mpenv {

// One allocation behind the three pointers: pool [R][capacity] snapshots
// (16-B aligned, 176 B each), then ticks [R][capacity] u32, then ranges [R][2]
// i32 (a table in memory: lanes of one wave index it by their slot's range).
struct PoolDev {
    mpenv_curriculum_snapshot *pool;
    uint32_t *ticks;
    int32_t R, capacity;
    int32_t period, stepLo, stepHi;
    uint32_t need, seed;
    uint32_t worldOffset; // the manager's world_id_offset
    const int32_t *ranges; // [R][2]: each range's first world in the batch and its number of worlds
};

// k_harvest over every slot of every range on `stream`, from the whole batch
// `s`.  fill 0: harvest tick `tick` (selection and filter of
// curriculum_core.h).  fill 1: the initial fill -- slot s of range r from world
// first_world(r) + s % num_worlds(r), unfiltered, tick 0.  The caller has checked
// that every range lies inside the batch.
int launchHarvest(const DevState &s, const PoolDev &p, uint32_t tick, int fill, void *stream);

} // namespace mpenv
