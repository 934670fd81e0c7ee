// league.h — what league.hip (k_league) and league.cpp (the mpenv_league_*
// entry points) share: the kernel's view of an enabled league and its launcher.
#pragma once

#include <hip/hip_runtime.h>

#include "engine.h"

namespace mpenv {

// One allocation behind all three pointers: table [P + 1][P + 1][8] i64, then
// weights [P + 1][P] i32, then draws [W] u32.
struct LeagueDev {
    long long *table;
    const int32_t *weights;
    uint32_t *draws;
    int32_t P;    // num_policies
    int32_t mode; // league_core.h kLeagueDraw*
    uint32_t seed;
    uint32_t worldOffset; // the manager's world_id_offset: world w draws as global world worldOffset + w
};

// k_league over the whole batch of `s` on `stream`: behind a step
// (initOnly 0: the worlds whose first agent reports done are recorded, then
// drawn) or behind an init (initOnly 1: every world draws, none is recorded)
int launchLeague(const DevState &s, const LeagueDev &lg, int initOnly, void *stream);

} // namespace mpenv
