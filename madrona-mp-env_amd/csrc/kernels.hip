// kernels.hip — the world-batched Zone step as hand-written gfx950 kernels.
//
// The reference runs ~40 ECS systems per step, each a device-wide
// ParallelForNode with a grid barrier in between (sim.cpp:5342-5842;
// NVRTC megakernel).  Every dependency between those systems is *within a
// world* (SURVEY.md §8e), so here a workgroup owns a tile of worlds and the
// system chain becomes LDS/L1-local __syncthreads() barriers.  The step is
// five kernels, k_sim here and the others in a file each (move.hip, vis.hip,
// obs.hip, lidar.hip):
//
//   k_move   lane = agent: bots, movement + sphere casts, aim, fall
//   k_sim    world tile, lane = agent: fire, damage,
//            respawn, heal, zone, breadcrumbs, match info, goals, explore,
//            rewards, done, reset  (sim.cpp:5347-5841 up to resetSystem)
//   k_vis    lane = (agent, opponent): frustum + line-of-sight rays
//            (opponentsWriteVisibilitySystem, sim.cpp:2526-2560)
//   k_obs    lane = agent: opponent masks + all observation tensors
//            (sim.cpp:2562-3052)
//   k_lidar  lane = ray: 80 lidar rays per agent (sim.cpp:3324-3506)
//
// All traversals read an LDS-resident copy of the BVH (geom_dev.h).  Every
// arithmetic expression follows the reference (and the CPU oracle) term by
// term with -ffp-contract=off so that results are bit-identical.
#include "curriculum_core.h"
#include "nav_dev.h"
#include "sight_dev.h"

#pragma clang fp contract(off)

namespace mpenv {

using namespace mp;

static_assert(kCrouch == mp::kPoseCrouch && kProne == mp::kPoseProne, "curriculum_core.h restates the pose ids");

// Zone and goal-region frames, once at scene upload (see FrameDev).
__global__ void k_scene_frames(SceneTables *tab)
{
    const int t = threadIdx.x;
    if (t < kMaxZones) {
        tab->zoneFrame[t] = makeFrameD(tab->zoneAABB[t].pMin, tab->zoneAABB[t].pMax, tab->zoneRot[t]);
    } else if (t >= 16 && t < 16 + 12) {
        const int r = (t - 16) / 3, k = (t - 16) % 3;
        const ZOBBDev &z = tab->goals[r].sub[k];
        tab->goalFrame[r][k] = makeFrameD(z.pMin, z.pMax, z.rotation);
    }
}

// The bots' goal is always a zone centroid: its NearestNavTri is computed
// once per zone at scene upload (same function, same input).
__global__ void k_zone_goals(SceneDev sc, int32_t *out)
{
    const int zi = threadIdx.x;
    if (zi >= sc.numZones) return;
    const AABB z = sc.zoneAABB[zi];
    const Vec3 center = (z.pMin + z.pMax) / 2.f; // as planAStarD forms it
    out[zi] = nearestNavTriD(sc, center);
}

// sim.cpp:1443-1615 fireSystem
// ---- event log (sim.cpp:23-39 logEvent; GameEvent types.hpp:729-760)
__device__ __forceinline__ uint64_t matchIdD(const DevState &S, const SceneDev &sc, int w)
{
    return ((uint64_t)(sc.worldOffset + (uint32_t)w) << 32) | (uint64_t)(uint32_t)S.episode[w];
}

__device__ __forceinline__ void putEventD(const DevState &S, const SceneDev &sc, int w, int slot, uint32_t type,
                                          int a, int b, int c16)
{
    mpenv_game_event ev;
    ev.type = type;
    ev.pad_ = 0;
    ev.match_id = matchIdD(S, sc, w);
    ev.step = (uint32_t)S.curStep[w];
    ev.a = (uint8_t)a;
    ev.b = (uint8_t)b;
    ev.c16 = (uint16_t)c16;
    S.events[(int64_t)w * S.evStride + slot] = ev;
}

__device__ __forceinline__ int playerIdD(const DevState &S, int i) { return (i / S.T) * kMaxTeamSize + i % S.T; }

// What fireD reads about its own agent, loaded before any of its stores.
struct FireIn {
    int32_t flags, mag0, mag1, fire, pose, respawn;
    float alive, hp, ayaw, apitch;
    Vec3 pos;
    RNG rng;
};

__device__ __forceinline__ FireIn fireLoadD(const DevState &S, int64_t g)
{
    FireIn f;
    f.flags = S.flags[g];
    f.alive = S.alive[g];
    f.mag0 = S.magazine[2 * g];
    f.mag1 = S.magazine[2 * g + 1];
    f.fire = S.discreteAction[4 * g + 2];
    f.pose = S.curPose[g];
    f.respawn = S.respawnSteps[g];
    f.hp = S.hp[g];
    f.ayaw = S.ayaw[g];
    f.apitch = S.apitch[g];
    f.pos = ldPos(S, g);
    f.rng = ldRng(S, g);
    return f;
}

// sim.cpp:1443-1615 fireSystem.  in: the agent's own inputs (fireLoadD);
// lpx / lpy / lpz, lhp, lrs: the world's agents' positions, hp and respawn
// counters in LDS (k_sim stages them), indexed from lb (the world's first
// lane).
template <class LBVH>
__device__ __forceinline__ void fireD(const DevState &S, const SceneDev &sc, const LBVH &bvh, int w, int i, const FireIn &in,
                                      const float *lpx, const float *lpy, const float *lpz, const float *lhp,
                                      const float *lrs, int lb)
{
    const int N = S.N;
    const int64_t g0 = (int64_t)w * N;
    const int64_t g = g0 + i;
    S.landedOn[g] = -1;
    S.firedT[g] = -kFltMax;
    int32_t flags = in.flags & ~(kFlagSuccessfulKill | kFlagReloadedFullMag);
    if (in.alive == 0.f) {
        S.flags[g] = flags;
        return;
    }
    int32_t mag0 = in.mag0, mag1 = in.mag1;
    const int fire = in.fire;
    if (fire == 2) {
        if (sc.eventsOn) putEventD(S, sc, w, 2 * i, MPENV_EVENT_RELOAD, playerIdD(S, i), mag0, 0);
        if (mag0 == c::kMagSize) flags |= kFlagReloadedFullMag;
        mag0 = c::kMagSize;
        mag1 = c::kReloadTime;
    }
    bool reloading = mag1 > 0;
    if (reloading) mag1 -= 1;
    bool should_fire = false;
    if (!reloading && mag0 > 0) should_fire = fire == 1;
    if (!should_fire) {
        S.magazine[2 * g] = mag0;
        S.magazine[2 * g + 1] = mag1;
        S.flags[g] = flags;
        return;
    }
    mag0 -= 1;
    S.magazine[2 * g] = mag0;
    S.magazine[2 * g + 1] = mag1;

    Vec3 fire_from = in.pos;
    fire_from.z += viewHeightD(in.pose);
    RNG rng = in.rng;
    float u1 = rngUniform(rng);
    float u2 = rngUniform(rng);
    stRng(S, g, rng);
    float z1 = sqrt_(-2.f * logf_(u1)) * cosf_(2.f * kPi * u2);
    float z2 = sqrt_(-2.f * logf_(u1)) * sinf_(2.f * kPi * u2);
    const float acc = c::kAccuracyScale;
    const float bias = 1.5f;
    float up_delta = fminD(fmaxD((z1 + bias) * acc, 0.f), 4.f * acc);
    float right_delta = fminD(fmaxD(z2 * acc, -4.f * acc), 4.f * acc);
    AimD a = computeAimD(in.ayaw + right_delta, in.apitch + up_delta);
    stAim(S, g, a);
    Vec3 fire_dir = rotateVec(a.rot, kFwd);

    WorldHit h = traceWorldD(bvh, lpx, lpy, lpz, lb, N, fire_from, fire_dir, i); // from its own axis
    if (S.stats) statAdd(S.stats + kStatShots, 1u);
    S.firedT[g] = h.hit ? h.t : kFltMax;
    bool success = h.hit;
    const int team = i / S.T, offset = i - team * S.T;
    if (h.entity == -1) {
        success = false;
    } else {
        const int tteam = h.entity / S.T;
        if (success && tteam == team) success = false;
        if (success && __float_as_int(lrs[lb + h.entity]) > 0) success = false;
    }
    if (success) {
        if (sc.eventsOn) putEventD(S, sc, w, 2 * i, MPENV_EVENT_PLAYER_SHOT, playerIdD(S, i), playerIdD(S, h.entity), 0);
        S.landedOn[g] = h.entity;
        if (lhp[lb + h.entity] <= c::kDmgPerBullet) {
            flags |= kFlagSuccessfulKill;
            if (sc.eventsOn) putEventD(S, sc, w, 2 * i + 1, MPENV_EVENT_KILL, playerIdD(S, i), playerIdD(S, h.entity), 0);
        }
        S.dmg[(int64_t)offset * S.dmgStride + g0 + h.entity] = c::kDmgPerBullet;
    }
    S.flags[g] = flags;
}

// sim.cpp:1794-1836 applyDmgSystem
// What the world lane's respawn reads about an agent after applyDmgD (k_sim
// hands it over in LDS).
struct DmgOut {
    bool alive;
    int32_t flags;
    Vec3 pos;
};

__device__ DmgOut applyDmgD(const DevState &S, int64_t g)
{
    // every input read before the first store (the damage slots are floats
    // like the stores between them, which would serialise the loads)
    int32_t flags = S.flags[g] & ~kFlagWasKilled;
    Vec3 pos = ldPos(S, g);
    const int rs = S.respawnSteps[g];
    float hp = S.hp[g];
    const bool was_alive = S.alive[g] == 1.f;
    int ah = S.autohealSteps[g];
    const int T = S.T;
    float dm[kMaxTeamSize];
    #pragma unroll
    for (int k = 0; k < kMaxTeamSize; k++) dm[k] = k < T ? S.dmg[(int64_t)k * S.dmgStride + g] : 0.f;
    if (rs > 0) S.respawnSteps[g] = rs - 1;
    int was_shot = 0;
    #pragma unroll
    for (int k = 0; k < kMaxTeamSize; k++) {
        if (k >= T) break;
        if (dm[k] > 0.f) was_shot += 1;
        hp -= dm[k];
        S.dmg[(int64_t)k * S.dmgStride + g] = 0.f;
    }
    if (was_shot > 0) ah = c::kOutOfCombatSteps;
    S.wasShot[g] = was_shot;
    if (was_alive && hp <= 0.f) flags |= kFlagWasKilled | kFlagHasDied;
    if (S.stats) {
        statAdd(S.stats + kStatHits, was_shot > 0 ? 1u : 0u);
        statAdd(S.stats + kStatKills, (was_alive && hp <= 0.f) ? 1u : 0u);
    }
    const bool dead = hp <= 0.f;
    if (dead) {
        hp = 0.f;
        S.alive[g] = 0.f;
        pos = v3(0, 0, 10000.f);
        stPos(S, g, pos);
        stVel(S, g, v3(0, 0, 0));
    } else {
        S.alive[g] = 1.f;
        // sim.cpp:1875-1890 autoHealSystem for the agents alive after the
        // damage (nothing between the two systems changes them; a
        // respawned agent's autoheal is spawnApplyD's)
        if (ah == 0 && hp < 100.f) hp = fminD(100.f, hp + c::kAutohealPerStep);
        else if (ah > 0) ah -= 1;
    }
    if (was_shot > 0 || !dead) S.autohealSteps[g] = ah;
    S.hp[g] = hp;
    S.flags[g] = flags;
    DmgOut o;
    o.alive = !dead;
    o.flags = flags;
    o.pos = pos;
    return o;
}

// ====================================================== spawning / reset
// utils.cpp:273-479 standardSpawnPoint (Zone task)
// Draw keys of an agent's fresh combat RNG (counters 0 .. kPreDraws-1),
// computed by the agent's own lane before a world reset so the world lane
// does not evaluate them one after another (k_sim, resetPreD).
constexpr int kPreDraws = 10;

// The spawn and reset code below is compiled per caller from three choices,
// each a small type: where "my world's agents" are read (MemAgents,
// LdsAgents), where an agent's draw keys come from (DrawnKeys, PreparedKeys)
// and what happens to a chosen spawn (SpawnApply, SpawnRecord).

// The world's agents in memory (one lane per world: k_construct and
// k_reset_only); tabA / tabB / tabC: the scene's aSpawns, bSpawns, commonRespawns.
struct MemAgents {
    const DevState &S;
    int64_t g0;
    const Spawn *tabA, *tabB, *tabC;
    __device__ Vec3 pos(int j) const { return ldPos(S, g0 + j); }
    __device__ bool alive(int j) const { return S.alive[g0 + j] != 0.f; }
    __device__ int32_t flags(int j) const { return S.flags[g0 + j]; }
    __device__ void markSpawned(int, Vec3) const {} // (the spawn's own stores are what later reads see)
};

// The world's agents in k_sim's LDS: positions [N][3] and alive bytes, both
// updated as agents spawn (the respawn scoring sees earlier spawns), each
// agent's flags before the spawn (as float bits), and LDS copies of the
// scene's spawn lists (aSpawns, bSpawns, commonRespawns).
struct LdsAgents {
    float *posL;
    uint8_t *aliveL;
    const float *flagsL;
    const Spawn *tabA, *tabB, *tabC;
    __device__ Vec3 pos(int j) const { return v3(posL[3 * j], posL[3 * j + 1], posL[3 * j + 2]); }
    __device__ bool alive(int j) const { return aliveL[j] != 0; }
    __device__ int32_t flags(int j) const { return __float_as_int(flagsL[j]); }
    __device__ void markSpawned(int j, Vec3 p) const
    {
        posL[3 * j] = p.x; posL[3 * j + 1] = p.y; posL[3 * j + 2] = p.z;
        aliveL[j] = 1;
    }
};

// Every draw from the agent's RNG in memory.
struct DrawnKeys {
    static constexpr bool kPrepared = false;
    __device__ RNG rng(const DevState &S, int64_t g, int) const { return ldRng(S, g); }
    __device__ RandKey next(int, RNG &r) const { return rngAdvance(r); }
};

// A world reset whose agents' lanes ran resetPreD: pre holds, per agent, its
// fresh RNG key, then the keys of its first kPreDraws draws (the same keys
// splitI(rng.key, ctr) the RNG would produce).
struct PreparedKeys {
    static constexpr bool kPrepared = true;
    const RandKey *pre;
    __device__ const RandKey *draws(int ai) const { return pre + ai * (kPreDraws + 1) + 1; }
    __device__ RNG rng(const DevState &, int64_t, int ai) const { return makeRNG(pre[ai * (kPreDraws + 1)]); }
    __device__ RandKey next(int ai, RNG &r) const
    {
        const RandKey k = r.ctr < (uint32_t)kPreDraws ? draws(ai)[r.ctr] : splitI(r.key, r.ctr);
        r.ctr += 1;
        return k;
    }
};

// A chosen spawn is applied at once by the world lane (spawnApplyD), or
// recorded for the agent's own lane to apply (k_sim, LDS): rec is the
// world's records, kSpawnRec floats per agent.
struct SpawnApply { static constexpr bool kRecord = false; };
struct SpawnRecord { static constexpr bool kRecord = true; float *rec; };

// World values the spawn loop reads once (not per agent).
struct SpawnWorld {
    int teamA, cz, episodeCurr;
    uint32_t curStep;
};

__device__ __forceinline__ SpawnWorld ldSpawnWorldD(const DevState &S, int w)
{
    return SpawnWorld{ S.teamA[w], S.curZone[w], S.episodeCurr[w], (uint32_t)S.curStep[w] };
}

// The world's dead agents as a bit mask (utils.cpp:767-780: fixed before the loop).
template <class Agents>
__device__ __forceinline__ uint32_t deadMaskD(const Agents &A, int N)
{
    uint32_t dead = 0;
    #pragma unroll 1
    for (int k = 0; k < N; k++)
        if (!A.alive(k)) dead |= 1u << k;
    return dead;
}

// Spawn indices taken so far in a world reset's loop, per team list (bits
// 0..127).  The reset cleared both lists just before (clearSpawnTrackD), so
// "tracker[idx] == curStep" holds exactly for the indices taken here.
struct SpawnTaken {
    uint64_t a0, a1, b0, b1;
};

// A chosen spawn: what spawnApplyD needs besides the agent's flags.  rngCtr
// >= 0: the agent's RNG counter after its spawn draws (its key is unchanged).
struct Spawned {
    Vec3 pt;
    float yaw, hp;
    int32_t mag, rngCtr;
};

// A Spawned as k_sim's world lane leaves it in LDS for the agent's lane:
// position, yaw, hp, then magazine and RNG counter as float bits.
constexpr int kSpawnRec = 8;

__device__ __forceinline__ void stSpawnRecD(float *r, const Spawned &s)
{
    r[0] = s.pt.x; r[1] = s.pt.y; r[2] = s.pt.z; r[3] = s.yaw;
    r[4] = s.hp; r[5] = __int_as_float(s.mag); r[6] = __int_as_float(s.rngCtr);
}

__device__ __forceinline__ Spawned ldSpawnRecD(const float *r)
{
    return Spawned{ v3(r[0], r[1], r[2]), r[3], r[4], __float_as_int(r[5]), __float_as_int(r[6]) };
}

// A point and yaw inside spawn region s from four draws (standardSpawnPoint's
// spawnAgent lambda).
__device__ __forceinline__ void spawnInRegionD(const Spawn &s, RandKey kx, RandKey ky, RandKey kz, RandKey kyaw,
                                               Vec3 &pt, float &yaw)
{
    const float x_rnd = keyUniform(kx), y_rnd = keyUniform(ky), z_rnd = keyUniform(kz), yaw_rnd = keyUniform(kyaw);
    const float x_min = s.region.pMin.x, x_diff = s.region.pMax.x - x_min;
    const float y_min = s.region.pMin.y, y_diff = s.region.pMax.y - y_min;
    const float z_min = s.region.pMin.z, z_diff = s.region.pMax.z - z_min;
    pt = v3(x_min + x_rnd * x_diff, y_min + y_rnd * y_diff, z_min + z_rnd * z_diff);
    yaw = s.yawMin + yaw_rnd * (s.yawMax - s.yawMin);
}

// spawnAgents' draws from the world RNG before its loop; returns use_middle.
__device__ __forceinline__ bool spawnPrologueD(const SceneDev &sc, RNG &base)
{
    // episodes[sampleI32(0, numEpisodes = 0)]: an empty range, the value is
    // 0 whatever the key -- only the counter advances
    base.ctr += 1;
    return (sc.simFlags & kFlagSpawnInMiddle) && rngUniform(base) < 0.5f;
}

// utils.cpp:819-837 LearnShooting: a standard spawn point replaced
__device__ __forceinline__ void learnShootingD(const SceneDev &sc, const SpawnWorld &sw, RNG &base, Vec3 &spawn_pt)
{
    if (!((sc.simFlags & kFlagEnableCurriculum) && sw.episodeCurr == 0)) return;
    const bool north = spawn_pt.y > 0.f;
    const float x = -700.f + rngUniform(base) * 1400.f;
    const float y = rngUniform(base) * 350.f;
    spawn_pt = v3(x, north ? y : -y, 0.f);
}

// The spawned agent's weapon, hp and magazine draws from the world RNG.
__device__ __forceinline__ void loadoutD(const SceneDev &sc, RNG &base, Spawned &sp)
{
    // sampleI32(0, numWeaponTypes = 1) is 0 whatever the key: advance only
    static_assert(c::kNumWeaponTypes == 1, "weapon draw shortcut assumes one weapon type");
    base.ctr += 1;
    sp.hp = 100.f;
    sp.mag = c::kMagSize;
    if (sc.simFlags & kFlagRandomizeHP) {
        int tenth = rngI32(base, 1, 11);
        sp.hp = float(tenth * 10);
        sp.mag = rngI32(base, 0, c::kMagSize);
    }
}

// One common respawn point's score for agent ai (utils.cpp:410-475 inside
// standardSpawnPoint's respawn branch): recently used points, points near
// any live agent, near live opponents, and near the zone score higher.
template <class Agents>
__device__ __forceinline__ float respawnScoreD(const DevState &S, const Agents &A, int s, int ai, int team,
                                               uint32_t last_used, uint32_t cur_step, Vec3 zone_center)
{
    const int N = S.N;
    float score = 0.f;
    uint32_t elapsed = (uint32_t)(c::kDeltaT * float(cur_step - last_used));
    const float elapsed_weight = 0.1f, dist_weight = 0.01f;
    if (elapsed < 3.f) score += elapsed_weight * (3.f - elapsed);
    Spawn sp = A.tabC[s];
    Vec3 spawn_pt = 0.5f * (sp.region.pMin + sp.region.pMax);
    #pragma unroll 1
    for (int j = 0; j < N; j++) {
        if (j == ai) continue;
        if (!A.alive(j)) continue;
        float dist = distance(spawn_pt, A.pos(j));
        if (dist < 4.f * c::kAgentRadius) {
            score += 100000.f;
        } else {
            if (j / S.T == team) continue;
            score += dist_weight * (1.f / dist);
        }
    }
    float dz = distance(spawn_pt, zone_center);
    if (dz < 100.f) score += 1000000.f;
    return score;
}

template <bool kRespawn, class Agents, class Keys>
__device__ __forceinline__ void standardSpawnPointD(const DevState &S, const SceneDev &sc, int w, int ai, bool use_middle,
                                                    RNG &rng, Vec3 &out_pt, float &out_yaw, const Agents &A,
                                                    const Keys &keys, const SpawnWorld &sw, SpawnTaken &tk)
{
    auto adv = [&]() { return keys.next(ai, rng); };
    auto spawnAgent = [&](const Spawn &s) {
        const RandKey kx = adv(), ky = adv(), kz = adv(), kyaw = adv();
        spawnInRegionD(s, kx, ky, kz, kyaw, out_pt, out_yaw);
    };
    const int team = ai / S.T;
    const uint32_t cur_step = sw.curStep;
    uint32_t *track = &S.spawnTrack[(int64_t)w * 3 * sc.spawnTrackLen];

    if (!kRespawn || sc.numCommon == 0) {
        const Spawn *options;
        uint32_t *tracker;
        int num_default, num_extra, num_spawns;
        const bool list_a = team == sw.teamA;
        if (list_a) {
            options = A.tabA;
            num_default = sc.numDefaultA;
            num_extra = sc.numA - sc.numDefaultA;
            tracker = track;
        } else {
            options = A.tabB;
            num_default = sc.numDefaultB;
            num_extra = sc.numB - sc.numDefaultB;
            tracker = track + sc.spawnTrackLen;
        }
        if (use_middle) {
            options += num_default;
            num_spawns = num_extra;
        } else {
            num_spawns = num_default;
        }
        if constexpr (Keys::kPrepared && !kRespawn) {
            if (rng.ctr == 0 && num_spawns <= 128) {
                // the agent's draw keys in one round of loads, the taken
                // indices from tk instead of the tracker
                RandKey k[kPreDraws];
                #pragma unroll
                for (int c = 0; c < kPreDraws; c++) k[c] = keys.draws(ai)[c];
                uint64_t &t0 = list_a ? tk.a0 : tk.b0, &t1 = list_a ? tk.a1 : tk.b1;
                auto taken = [&](int idx) { return (((idx < 64 ? t0 : t1) >> (idx & 63)) & 1ull) != 0; };
                int init_idx = keyI32(k[5], 0, num_spawns), used = 6;
                #pragma unroll
                for (int t = 4; t >= 0; t--) {
                    const int idx = keyI32(k[t], 0, num_spawns);
                    if (!taken(idx)) { init_idx = idx; used = t + 1; }
                }
                // draws used .. used + 3 position the agent
                RandKey kk[4];
                #pragma unroll
                for (int j = 0; j < 4; j++) {
                    kk[j] = k[6 + j];
                    #pragma unroll
                    for (int t = 5; t >= 1; t--)
                        if (used == t) kk[j] = k[t + j];
                }
                rng.ctr = (uint32_t)(used + 4);
                spawnInRegionD(options[init_idx], kk[0], kk[1], kk[2], kk[3], out_pt, out_yaw);
                (init_idx < 64 ? t0 : t1) |= 1ull << (init_idx & 63);
                tracker[init_idx] = cur_step;
                return;
            }
        }
        int init_idx = -1;
        for (int k = 0; k < 5; k++) {
            int idx = keyI32(adv(), 0, num_spawns);
            if (tracker[idx] == cur_step) continue;
            init_idx = idx;
            break;
        }
        if (init_idx == -1) init_idx = keyI32(adv(), 0, num_spawns);
        spawnAgent(options[init_idx]);
        tracker[init_idx] = cur_step;
        return;
    }

    uint32_t *rtrack = track + 2 * sc.spawnTrackLen;
    AABB za = sc.tab->zoneAABB[sw.cz];
    Vec3 zone_center = 0.5f * (za.pMin + za.pMax);
    float best_score = kFltMax;
    int best_idx = -1;
    // the next entry's tracker load is in flight during this one's scoring
    uint32_t next_used = sc.numCommon > 0 ? rtrack[0] : 0u;
    for (int s = 0; s < sc.numCommon; s++) {
        const uint32_t last_used = next_used;
        if (s + 1 < sc.numCommon) next_used = rtrack[s + 1];
        if (last_used == cur_step) continue;
        const float score = respawnScoreD(S, A, s, ai, team, last_used, cur_step, zone_center);
        if (score < best_score) {
            best_idx = s;
            best_score = score;
        }
    }
    if (best_idx < 0) best_idx = 0;
    spawnAgent(A.tabC[best_idx]);
    rtrack[best_idx] = cur_step;
}

// AgentPolicy idx clamped to the 8 sub-zones (sim.cpp:1996-1997)
__device__ __forceinline__ int subZoneIndexD(const DevState &S, int64_t g)
{
    const int p = S.policy[g];
    return p < 0 ? 0 : (p > 7 ? 7 : p);
}

// The zone box of zone cz in its own frame (spawnAgents' in-zone test).
struct ZoneBox {
    AABB box;
    Vec3 center;
    Quat toZone;
};

__device__ __forceinline__ ZoneBox zoneBoxD(const SceneDev &sc, int cz)
{
    ZoneBox z;
    z.box = sc.tab->zoneAABB[cz];
    z.center = (z.box.pMax + z.box.pMin) / 2.f;
    z.toZone = qinv(angleAxis(sc.tab->zoneRot[cz], kUp));
    z.box.pMin = rotateVec(z.toZone, z.box.pMin);
    z.box.pMax = rotateVec(z.toZone, z.box.pMax);
    return z;
}

// A spawned agent's own stores once its spawn is chosen (the rest of
// utils.cpp:734-948's loop body).  flags: the agent's flags before the
// spawn.  Run by the world lane, or (k_sim) by the agent's own lane from the
// world lane's record.  A reset (!is_respawn) also stores the agent's start
// position (sx, sy, sz: resetPersistentEntities sets them from the spawn).
__device__ __forceinline__ void spawnApplyD(const DevState &S, const SceneDev &sc, int64_t g, bool is_respawn,
                                            const Spawned &sp, int32_t flags, const ZoneBox &zb)
{
    Vec3 spawn_pt = sp.pt;
    stPos(S, g, spawn_pt);
    if (!is_respawn) { S.sx[g] = spawn_pt.x; S.sy[g] = spawn_pt.y; S.sz[g] = spawn_pt.z; }
    if (sp.rngCtr >= 0) S.rngCtr[g] = sp.rngCtr;
    stRot(S, g, qnormalize(angleAxis(sp.yaw, kUp)));
    stAim(S, g, computeAimD(sp.yaw, 0.f));
    stVel(S, g, v3(0.f, 0.f, 0.f));
    S.weapon[g] = 0;
    // a respawn is followed by autoHealSystem (sim.cpp:1875-1890; alive, no
    // autoheal countdown)
    float hp = sp.hp;
    if (is_respawn && hp < 100.f) hp = fminD(100.f, hp + c::kAutohealPerStep);
    S.hp[g] = hp;
    S.magazine[2 * g] = sp.mag;
    S.magazine[2 * g + 1] = 0;
    S.respawnSteps[g] = is_respawn ? 0 : c::kRespawnInvincibleSteps;
    S.autohealSteps[g] = 0;
    {
        Vec3 pz = rotateVec(zb.toZone, spawn_pt);
        spawn_pt.z += c::kStandHeight / 2.f;
        flags = aabbContains(zb.box, pz) ? (flags | kFlagInZone) : (flags & ~kFlagInZone);
        S.minDistZone[g] = distance(spawn_pt, zb.center);
    }
    if (sc.simFlags & kFlagSubZones) {
        // utils.cpp:906-926: spawn_pt already carries the +standHeight/2
        // of the zone block and receives it a second time
        const ZOBBDev &sz = sc.tab->subZones[subZoneIndexD(S, g)];
        AABB za = { sz.pMin, sz.pMax };
        Vec3 sub_center = (za.pMax + za.pMin) / 2.f;
        Quat to_sub = qinv(angleAxis(sz.rotation, kUp));
        za.pMin = rotateVec(to_sub, za.pMin);
        za.pMax = rotateVec(to_sub, za.pMax);
        Vec3 pz = rotateVec(to_sub, spawn_pt);
        spawn_pt.z += c::kStandHeight / 2.f;
        flags = aabbContains(za, pz) ? (flags | kFlagInSubZone) : (flags & ~kFlagInSubZone);
        S.minDistSub[g] = distance(spawn_pt, sub_center);
    }
    S.flags[g] = flags;
    S.curPose[g] = kStand; S.tgtPose[g] = kStand; S.transRem[g] = 0;
    S.maxVel[g] = c::kMaxWalkVelocity;
    S.dyv[g] = 0.f; S.dpv[g] = 0.f;
    S.alive[g] = 1.f;
}

// utils.cpp:734-948 spawnAgents over the agents in dead_mask, drawing from
// the world RNG base (the caller loads and stores it).
template <bool kRespawn, class Agents, class Keys, class Sink>
__device__ __forceinline__ void spawnAgentsD(const DevState &S, const SceneDev &sc, int w, const Agents &A,
                                             const Keys &keys, const Sink &sink, uint32_t dead_mask,
                                             const SpawnWorld &sw, RNG &base)
{
    if (dead_mask == 0) return;
    const int N = S.N;
    const int64_t g0 = (int64_t)w * N;
    const bool use_middle = spawnPrologueD(sc, base);
    // the zone box in its own frame, once for every agent (recorded spawns:
    // the agents' lanes compute it)
    ZoneBox zb;
    if constexpr (!Sink::kRecord) zb = zoneBoxD(sc, sw.cz);
    SpawnTaken tk = { 0ull, 0ull, 0ull, 0ull };

    #pragma unroll 1
    for (int ai = 0; ai < N; ai++) {
        if (!(dead_mask & (1u << ai))) continue;
        const int64_t g = g0 + ai;
        Spawned sp;
        sp.rngCtr = -1;
        if ((sc.simFlags & kFlagHardcodedSpawns) && !kRespawn) {
            // utils.cpp:480-650 hardcodedSpawnPoint
            const int team = ai / S.T;
            hardcodedSpawn((team == sw.teamA ? 0 : 3) + (ai - team * S.T), sp.pt, sp.yaw);
        } else if (sc.simFlags & kFlagNavmeshSpawn) {
            // utils.cpp:807-809
            sp.pt = navSamplePoint(sc.navTris, sc.navCdf, sc.numNavTris, rngAdvance(base));
            sp.yaw = rngUniform(base) * 2.f * kPi;
        } else {
            RNG rng = keys.rng(S, g, ai);
            standardSpawnPointD<kRespawn>(S, sc, w, ai, use_middle, rng, sp.pt, sp.yaw, A, keys, sw, tk);
            sp.rngCtr = (int32_t)rng.ctr; // (the key is unchanged)
            learnShootingD(sc, sw, base, sp.pt);
        }
        // (every agent of a reset is dead: nothing scores against positions)
        if constexpr (kRespawn) A.markSpawned(ai, sp.pt);
        loadoutD(sc, base, sp);
        if constexpr (Sink::kRecord) stSpawnRecD(sink.rec + ai * kSpawnRec, sp);
        else spawnApplyD(S, sc, g, kRespawn, sp, A.flags(ai), zb);
    }
}

// k_sim's respawn on the world lane: spawnAgents over the dead agents.
template <class Sink>
__device__ __forceinline__ void respawnSerialD(const DevState &S, const SceneDev &sc, int w, const LdsAgents &A,
                                               const Sink &sink)
{
    const uint32_t dead = deadMaskD(A, S.N);
    if (dead == 0) return;
    RNG base = ldWRng(S, w);
    spawnAgentsD<true>(S, sc, w, A, DrawnKeys{}, sink, dead, ldSpawnWorldD(S, w), base);
    stWRng(S, w, base);
}

// k_sim's respawn (spawnAgents with is_respawn, common respawn points, no
// navmesh spawns) with each dead agent's candidate scoring spread over its
// world's N lanes: one dead agent per world per round, in agent order; every
// lane scores candidates i, i + N, ... with respawnScoreD, the world lane
// takes the lowest score (lowest index on ties, as the sequential strict-<
// scan does), draws the spawn point and writes the agent's record (the
// agent's lane applies it).
// Points taken earlier this step are tracked in LDS (usedL) next to the
// tracker loads, so no lane reads back a tracker entry another lane stored.
// Called by every thread of the block (block barriers).  coop: LDS scratch,
// 4 floats per thread.
__device__ __forceinline__ void respawnCoopD(const DevState &S, const SceneDev &sc, int w, int i, int wl, bool act,
                                             const LdsAgents &A, float *rec, float *coop)
{
    const int N = S.N, T = S.T;
    const int B = (int)blockDim.x;
    float *const bestS = coop;          // per lane: best score
    float *const bestI = coop + B;      // per lane: its index (float bits)
    float *const curA = coop + 2 * B;   // per world: the agent this round (float bits)
    float *const usedL = coop + 3 * B;  // per world: 2 x 32 bits of points taken this step
    const bool wl0 = act && i == 0;
    uint32_t rem = 0;
    RNG base;
    SpawnWorld sw;
    if (wl0) {
        rem = deadMaskD(A, N);
        if (rem) {
            base = ldWRng(S, w);
            sw = ldSpawnWorldD(S, w);
            (void)spawnPrologueD(sc, base);
        }
        usedL[2 * wl] = 0.f;
        usedL[2 * wl + 1] = 0.f;
    }
    const uint32_t *rtrack = act ? &S.spawnTrack[(int64_t)w * 3 * sc.spawnTrackLen + 2 * sc.spawnTrackLen] : nullptr;
    uint32_t cur_step = 0u;
    #pragma unroll 1
    for (;;) {
        int ai = -1;
        if (wl0) {
            ai = rem ? __builtin_ctz(rem) : -1;
            curA[wl] = __int_as_float(ai);
        }
        if (!__syncthreads_or(ai >= 0)) break;
        const int a = act ? __float_as_int(curA[wl]) : -1;
        if (a >= 0) {
            // (read only in blocks with a respawn: most launches have none)
            cur_step = (uint32_t)S.curStep[w];
            const AABB za = sc.tab->zoneAABB[S.curZone[w]];
            const Vec3 zone_center = 0.5f * (za.pMin + za.pMax);
            const uint32_t used0 = (uint32_t)__float_as_int(usedL[2 * wl]), used1 = (uint32_t)__float_as_int(usedL[2 * wl + 1]);
            const int team = a / T;
            float bs = kFltMax;
            int bi = -1;
            #pragma unroll 1
            for (int sp = i; sp < sc.numCommon; sp += N) {
                const bool taken = ((sp < 32 ? used0 : used1) >> (sp & 31)) & 1u;
                const uint32_t last_used = taken ? cur_step : rtrack[sp];
                if (last_used == cur_step) continue;
                const float score = respawnScoreD(S, A, sp, a, team, last_used, cur_step, zone_center);
                if (score < bs) {
                    bs = score;
                    bi = sp;
                }
            }
            bestS[threadIdx.x] = bs;
            bestI[threadIdx.x] = __int_as_float(bi);
        }
        __syncthreads();
        if (wl0 && ai >= 0) {
            float best = kFltMax;
            int best_idx = -1;
            for (int k = 0; k < N; k++) {
                const int s_k = __float_as_int(bestI[wl * N + k]);
                if (s_k < 0) continue;
                const float sc_k = bestS[wl * N + k];
                if (sc_k < best || (sc_k == best && s_k < best_idx)) {
                    best = sc_k;
                    best_idx = s_k;
                }
            }
            if (best_idx < 0) best_idx = 0;
            // standardSpawnPoint's spawnAgent(best_idx), the agent's RNG
            RNG rng = ldRng(S, (int64_t)w * N + ai);
            const RandKey kx = rngAdvance(rng), ky = rngAdvance(rng), kz = rngAdvance(rng), kyaw = rngAdvance(rng);
            Spawned sp;
            spawnInRegionD(A.tabC[best_idx], kx, ky, kz, kyaw, sp.pt, sp.yaw);
            sp.rngCtr = (int32_t)rng.ctr;
            S.spawnTrack[(int64_t)w * 3 * sc.spawnTrackLen + 2 * sc.spawnTrackLen + best_idx] = cur_step;
            if (best_idx < 32) usedL[2 * wl] = __int_as_float(__float_as_int(usedL[2 * wl]) | (int)(1u << best_idx));
            else usedL[2 * wl + 1] = __int_as_float(__float_as_int(usedL[2 * wl + 1]) | (int)(1u << (best_idx & 31)));
            learnShootingD(sc, sw, base, sp.pt);
            A.markSpawned(ai, sp.pt);
            loadoutD(sc, base, sp);
            stSpawnRecD(rec + ai * kSpawnRec, sp);
            rem &= rem - 1u;
            if (rem == 0) stWRng(S, w, base);
        }
        __syncthreads();
    }
}

// level_gen.cpp:330-582 resetPersistentEntities
// resetPersistentEntities, agent i's own part (level_gen.cpp:330-370):
// position, combat RNG split_i(episodeKey, i + 1), combat flags, last-known
// observations, breadcrumb state.
// Returns the agent's flags after the reset.
__device__ __forceinline__ int32_t resetAgentD(const DevState &S, int64_t g, RandKey agent_key)
{
    stPos(S, g, v3(kFltMax, kFltMax, kFltMax));
    stRng(S, g, makeRNG(agent_key));
    S.landedOn[g] = -1;
    S.respawnSteps[g] = 0;
    S.autohealSteps[g] = 0;
    S.wasShot[g] = 0;
    S.firedT[g] = -kFltMax;
    // successfulKill/wasKilled/hasDied/reloadedFullMag = false
    const int32_t flags = S.flags[g] & (kFlagInZone | kFlagInSubZone);
    S.flags[g] = flags;
    S.alive[g] = 0.f;
    float4 *lk = reinterpret_cast<float4 *>(&S.lkObs[g * 6 * kOtherObs]);
    for (int k = 0; k < 6 * kOtherObs / 4; k++) lk[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < 18; k++) S.lkPos[g * 18 + k] = -1000.f;
    S.bcPenalty[g] = 0.f;
    S.bcLast[g] = -1;
    S.bcSteps[g] = 0;
    return flags;
}

// The reset of a world's spawn-usage tracker: entries first, first + stride, ...
__device__ __forceinline__ void clearSpawnTrackD(const DevState &S, const SceneDev &sc, int w, int first, int stride)
{
    uint32_t *track = &S.spawnTrack[(int64_t)w * 3 * sc.spawnTrackLen];
    for (int k = first; k < 3 * sc.spawnTrackLen; k += stride) track[k] = 0xFFFFFFFFu;
}

// The reset agent's stores after its spawn.
__device__ __forceinline__ void resetAgentTailD(const DevState &S, int64_t g)
{
    for (int k = 0; k < 4; k++) S.discreteAction[4 * g + k] = 0;
    S.aimAction[2 * g] = 0.f; S.aimAction[2 * g + 1] = 0.f;
    S.newCells[g] = 0;
    float *rc = &S.rewardCoefs[9 * g];
    rc[0] = 0.f; rc[1] = 0.5f; rc[2] = 0.005f; rc[3] = 0.05f; rc[4] = 0.01f;
    rc[5] = 0.1f; rc[6] = 0.0005f; rc[7] = 1.f; rc[8] = 0.1f;
}

// PreparedKeys: every agent's resetAgentD and its share of the tracker clear
// already ran on its own lane (resetPreD).  SpawnRecord (only without
// curriculum snapshots, which rewrite agents after the spawn): the agents'
// lanes apply the records and do resetAgentTailD.
// sw, base: the world values and RNG initWorld has just stored.
template <class Agents, class Keys, class Sink>
__device__ __forceinline__ void resetPersistentEntitiesD(const DevState &S, const SceneDev &sc, int w, RandKey episode_key,
                                                         const Agents &A, const Keys &keys, const Sink &sink,
                                                         const SpawnWorld &sw, RNG &base)
{
    const int N = S.N;
    const int64_t g0 = (int64_t)w * N;
    if constexpr (!Keys::kPrepared) {
        #pragma unroll 1
        for (int i = 0; i < N; i++) resetAgentD(S, g0 + i, splitI(episode_key, (uint32_t)(i + 1)));
        clearSpawnTrackD(S, sc, w, 0, 1);
    }
    // every agent is dead here (resetAgentD)
    spawnAgentsD<false>(S, sc, w, A, keys, sink, (1u << N) - 1u, sw, base);

    #pragma unroll 1
    for (int i = 0; i < N; i++) {
        if constexpr (!Sink::kRecord) resetAgentTailD(S, g0 + i);
        // level_gen.cpp:427-446: nine discarded coefficient draws.
        base.ctr += 9;
    }
    // GoalRegionsState (level_gen.cpp:472-485)
    S.goalMin0[w] = kFltMax;
    S.goalMin1[w] = kFltMax;
    S.goalTeam0[w] = 0.f;
    S.goalTeam1[w] = 0.f;

    // level_gen.cpp:498-580: start from a recorded match state half the time
    // (not in eval mode); the uniform is drawn whenever snapshots exist
    if (sc.numSnapshots > 0 && rngUniform(base) < 0.5f && !S.trainCtrl[0]) {
        const mpenv_curriculum_snapshot &sn = sc.curriculum[rngI32(base, 0, sc.numSnapshots)];
        S.curZone[w] = sn.cur_zone;
        if (sn.cur_zone_controller == -1) {
            S.controlling[w] = -1;
            S.captured[w] = 0;
        } else {
            S.captured[w] = 1;
            S.controlling[w] = sn.cur_zone_controller;
            S.stepsUntilPoint[w] = sn.steps_until_point;
            S.zoneSteps[w] = sn.zone_steps_remaining;
        }
        S.curStep[w] = sn.step;
        const int half = N / 2;
        const int team_a = S.teamA[w];
        #pragma unroll 1
        for (int i = 0; i < N; i++) {
            const int j = team_a == 0 ? i : (i < half ? half + i : i - half);
            const int64_t g = g0 + j;
            const mpenv_packed_player &p = sn.players[i];
            stPos(S, g, v3((float)p.pos[0], (float)p.pos[1], (float)p.pos[2]));
            const AimD aim = computeAimD((float)p.yaw * kPi / 32768.f, (float)p.pitch * kPi / 32768.f);
            stAim(S, g, aim);
            stRot(S, g, qnormalize(angleAxis(aim.yaw, kUp)));
            S.hp[g] = (float)p.hp;
            S.magazine[2 * g] = p.mag_num_bullets;
            S.magazine[2 * g + 1] = p.is_reloading;
            if (p.flags & 4) { S.curPose[g] = kCrouch; S.tgtPose[g] = kCrouch; S.transRem[g] = 0; }
            if (p.flags & 8) { S.curPose[g] = kProne; S.tgtPose[g] = kProne; S.transRem[g] = 0; }
        }
    }
    stWRng(S, w, base);
}

// sim.cpp:732-833 initWorld
template <class Agents, class Keys, class Sink>
__device__ __forceinline__ void initWorldD(const DevState &S, const SceneDev &sc, int w, bool triggered_reset,
                                           const int32_t *tc, const Agents &A, const Keys &keys, const Sink &sink)
{
    const uint32_t world_id = sc.worldOffset + (uint32_t)w;
    S.matchValid[w] = 1; // matchID = worldID << 32 | curEpisodeIdx (sim.cpp:736-738)
    SpawnWorld sw;
    sw.episodeCurr = S.worldCurr[w];
    S.episodeCurr[w] = sw.episodeCurr;
    const uint32_t ep = (uint32_t)S.episode[w];
    RandKey episode_key = splitI(sc.initRandKey, ep, world_id);
    RNG base = makeRNG(splitI(episode_key, 0));
    bool flip = false;
    if (tc[2]) flip = rngUniform(base) < 0.5f;
    sw.teamA = flip ? 1 : 0;
    S.teamA[w] = sw.teamA;
    const int32_t cur_step = (triggered_reset && tc[1]) ? rngI32(base, 0, c::kEpisodeLen - 1) : 0;
    S.curStep[w] = cur_step;
    sw.curStep = (uint32_t)cur_step;
    S.finished[w] = 0;
    const float use_prob = 1.0f;
    const float tier_probs[5] = { 0.f, 0.f, 0.3f, 0.3f, 0.4f };
    S.spawnCurriculum[w] = rngUniform(base) < use_prob ? 1 : 0;
    float cdf[5];
    float running = 0.f;
    for (int i = 0; i < 5; i++) { running += tier_probs[i]; cdf[i] = running; }
    float sel = running * rngUniform(base);
    for (int i = 0; i < 5; i++) {
        if (sel < cdf[i]) { S.curTier[w] = i; break; }
    }
    S.curSpawnIdx[w] = rngI32(base, 0, 0);
    if (sc.simFlags & kFlagHardcodedSpawns) (void)rngI32(base, 0, 4);
    sw.cz = rngI32(base, 0, sc.numZones);
    if (sc.task == MPENV_TASK_ZONE_CAPTURE_DEFEND) sw.cz = 3; // sim.cpp:822-825
    S.curZone[w] = sw.cz;
    S.controlling[w] = -1;
    S.contested[w] = 0;
    S.captured[w] = 0;
    S.earned[w] = 0;
    S.zoneSteps[w] = c::kNumStepsPerZone;
    S.stepsUntilPoint[w] = c::kZonePointInterval;
    S.subState[w] = 0; // every sub-zone: controlling -1, not contested / captured (sim.cpp:815-820)
    stWRng(S, w, base);
    resetPersistentEntitiesD(S, sc, w, episode_key, A, keys, sink, sw, base);
    S.filtAct0[w] = 0; S.filtAct1[w] = 0;
    S.filtMatched0[w] = 0; S.filtMatched1[w] = 0;
}

// sim.cpp:835-872 resetSystem
__device__ __forceinline__ bool resetDueD(const DevState &S, const SceneDev &sc, int w)
{
    return S.reset[w] != 0 || (sc.autoReset && S.finished[w]);
}

// The per-agent half of a coming world reset, on the agent's own lane
// (k_sim, before resetSystemD): the episode key initWorld will derive, the
// agent's combat RNG key split_i(episodeKey, i + 1) and its first kPreDraws
// draw keys into pre[0], pre[1..] (PreparedKeys), the agent's
// resetPersistentEntities stores, and its share of the spawn-usage tracker
// reset.
// Returns the agent's flags after its reset.
__device__ __forceinline__ int32_t resetPreD(const DevState &S, const SceneDev &sc, int w, int i, RandKey *pre)
{
    const uint32_t world_id = sc.worldOffset + (uint32_t)w;
    const uint32_t ep = (uint32_t)S.episodeCounter[w]; // the episode resetSystemD is about to start
    const RandKey episode_key = splitI(sc.initRandKey, ep, world_id);
    const RandKey key = splitI(episode_key, (uint32_t)(i + 1));
    pre[0] = key;
    for (int c = 0; c < kPreDraws; c++) pre[1 + c] = splitI(key, (uint32_t)c);
    const int32_t flags = resetAgentD(S, (int64_t)w * S.N + i, key);
    clearSpawnTrackD(S, sc, w, i, S.N);
    return flags;
}

template <class Agents, class Keys, class Sink>
__device__ __forceinline__ void resetSystemD(const DevState &S, const SceneDev &sc, int w, const Agents &A,
                                             const Keys &keys, const Sink &sink)
{
    const int32_t force = S.reset[w];
    if (!resetDueD(S, sc, w)) return;
    S.reset[w] = 0;
    const int32_t ep = S.episodeCounter[w];
    S.episode[w] = ep;
    S.episodeCounter[w] = ep + 1;
    if (sc.simFlags & kFlagEnableCurriculum) {
        if ((uint32_t)ep < 50) {
            RNG base = ldWRng(S, w);
            if (rngUniform(base) < ((uint32_t)ep + 1) / (float)50) S.worldCurr[w] = 1;
            else S.worldCurr[w] = 0;
            stWRng(S, w, base);
        } else {
            S.worldCurr[w] = 1;
        }
    }
    initWorldD(S, sc, w, force == 1, S.trainCtrl, A, keys, sink);
}

// ====================================================== per-world systems
// sim.cpp:1892-1976 zoneSystem, in three parts so that the step kernel can
// run the middle one on every agent's lane: the world lane rotates the zone
// (zonePreD), each agent is tested against the zone box (zoneInD), and the
// world lane counts the teams and stores (zonePostD).
struct ZonePre {
    int cz, ctrl, zsr, sup;
    bool captured;
};

__device__ __forceinline__ ZonePre zonePreD(const DevState &S, const SceneDev &sc, int w)
{
    const int N = S.N;
    const int64_t g0 = (int64_t)w * N;
    ZonePre z;
    z.cz = S.curZone[w];
    z.ctrl = S.controlling[w];
    z.zsr = S.zoneSteps[w];
    z.sup = S.stepsUntilPoint[w];
    z.captured = S.captured[w] != 0;
    if (z.ctrl != -1) z.zsr -= 1;
    if (z.zsr == 0) {
        z.cz += 1;
        if (z.cz == sc.numZones) z.cz = 0;
        z.captured = false;
        z.zsr = c::kNumStepsPerZone;
        z.sup = c::kZonePointInterval;
        AABB za = sc.tab->zoneAABB[z.cz];
        Vec3 center = (za.pMax + za.pMin) / 2.f;
#pragma unroll 1
        for (int i = 0; i < N; i++) S.minDistZone[g0 + i] = distance(ldPos(S, g0 + i), center);
    }
    return z;
}

__device__ __forceinline__ bool zoneInD(const DevState &S, const SceneDev &sc, int cz, int64_t g)
{
    const FrameDev &f = sc.tab->zoneFrame[cz];
    AABB za;
    za.pMin = f.pMin;
    za.pMax = f.pMax;
    Vec3 p = ldPos(S, g);
    p.z += c::kStandHeight / 2.f;
    const bool in = aabbContains(za, rotateVec(f.toFrame, p));
    setFlag(S, g, kFlagInZone, in);
    return in;
}

__device__ __forceinline__ void zonePostD(const DevState &S, int w, ZonePre z, int na, int nb)
{
    z.sup -= 1;
    bool contested = na > 0 && nb > 0;
    if (contested || (na == 0 && nb == 0)) {
        z.ctrl = -1;
        z.captured = false;
        z.sup = c::kZonePointInterval;
    } else if (na > 0 && nb == 0) {
        if (z.ctrl != 0) { z.ctrl = 0; z.captured = false; z.sup = c::kZonePointInterval; }
    } else if (na == 0 && nb > 0) {
        if (z.ctrl != 1) { z.ctrl = 1; z.captured = false; z.sup = c::kZonePointInterval; }
    }
    S.curZone[w] = z.cz;
    S.controlling[w] = z.ctrl;
    S.zoneSteps[w] = z.zsr;
    S.stepsUntilPoint[w] = z.sup;
    S.captured[w] = z.captured ? 1 : 0;
    S.contested[w] = contested ? 1 : 0;
}

// zoneSystem on one lane (the replay path)
__device__ void zoneSystemD(const DevState &S, const SceneDev &sc, int w)
{
    const int64_t g0 = (int64_t)w * S.N;
    const ZonePre z = zonePreD(S, sc, w);
    int na = 0, nb = 0;
#pragma unroll 1
    for (int i = 0; i < S.N; i++) {
        if (!zoneInD(S, sc, z.cz, g0 + i)) continue;
        if (i / S.T == 0) na += 1;
        else nb += 1;
    }
    zonePostD(S, w, z, na, nb);
}

// SubZone state packed 4 bits per sub-zone k at bit 4k: controlling team + 1,
// contested << 2, captured << 3 (the DEBUG_WORLD_I32 layout).
__device__ __forceinline__ int subCtrlD(uint32_t st, int k) { return (int)((st >> (4 * k)) & 3u) - 1; }

// sim.cpp:1978-2041 subzoneSystem over sub-zones 0..7
__device__ void subzoneSystemD(const DevState &S, const SceneDev &sc, int w)
{
    const int N = S.N;
    const int64_t g0 = (int64_t)w * N;
    uint32_t st = (uint32_t)S.subState[w];
    for (int k = 0; k < 8; k++) {
        const ZOBBDev &sz = sc.tab->subZones[k];
        AABB za = { sz.pMin, sz.pMax };
        Quat to_zone = qinv(angleAxis(sz.rotation, kUp));
        za.pMin = rotateVec(to_zone, za.pMin);
        za.pMax = rotateVec(to_zone, za.pMax);
        int na = 0, nb = 0;
        #pragma unroll 1
        for (int i = 0; i < N; i++) {
            const int64_t g = g0 + i;
            if (subZoneIndexD(S, g) != k) continue;
            Vec3 p = ldPos(S, g);
            p.z += c::kStandHeight / 2.f;
            const bool in = aabbContains(za, rotateVec(to_zone, p));
            setFlag(S, g, kFlagInSubZone, in);
            if (!in) continue;
            S.minDistSub[g] = 0.f;
            if (i / S.T == 0) na += 1;
            else nb += 1;
        }
        int ctrl = subCtrlD(st, k);
        bool captured = (st >> (4 * k + 3)) & 1u;
        const bool contested = na > 0 && nb > 0;
        if (contested || (na == 0 && nb == 0)) {
            ctrl = -1;
            captured = false;
        } else if (na > 0 && nb == 0) {
            if (ctrl != 0) { ctrl = 0; captured = false; }
        } else if (na == 0 && nb > 0) {
            if (ctrl != 1) { ctrl = 1; captured = false; }
        }
        const uint32_t nib = (uint32_t)(ctrl + 1) | (contested ? 4u : 0u) | (captured ? 8u : 0u);
        st = (st & ~(0xFu << (4 * k))) | (nib << (4 * k));
    }
    S.subState[w] = (int32_t)st;
}

// sim.cpp:4845-4889 leaveBreadcrumbsSystem, agent part: refresh own last
// crumb or request a new one (returns true; appended in agent order by the
// world lane, the requests handed over in LDS).  The penalty's reset to 0
// is crumbRoundsD's starting value (the two always run together).
__device__ bool leaveBreadcrumbAgentD(const DevState &S, int w, int64_t g)
{
    const Vec3 pos = ldPos(S, g);
    const int32_t last = S.bcLast[g];
    bool updated = false;
    if (last != -1) {
        float4 *cr = crumbPtr(S, w);
        const int n = S.numCrumbs[w];
        // the first crumb with id `last`, its ids read 8 at a time (one
        // round of loads per 8 crumbs; past the end re-reads the last)
        constexpr int kIds = 8;
        int hit = -1;
        #pragma unroll 1
        for (int k0 = 0; k0 < n && hit < 0; k0 += kIds) {
            int id[kIds];
            #pragma unroll
            for (int j = 0; j < kIds; j++) id[j] = __float_as_int(cr[2 * min(k0 + j, n - 1) + 1].z);
            #pragma unroll
            for (int j = kIds - 1; j >= 0; j--)
                if (k0 + j < n && id[j] == last) hit = k0 + j;
        }
        if (hit >= 0) {
            const float4 p = cr[2 * hit];
            if (distance(pos, v3(p.x, p.y, p.z)) < c::kAgentRadius * 4) {
                cr[2 * hit].w = 1.f;
                updated = true;
                S.bcSteps[g] = 0;
            }
        }
    }
    bool request = false;
    if (!updated) {
        int steps = S.bcSteps[g] + 1;
        if (steps > 10) {
            request = true;
            steps = 0;
        }
        S.bcSteps[g] = steps;
    }
    return request;
}

// World part of leaveBreadcrumbsSystem: append requested crumbs in agent
// order (req: bit i = agent i asked, from leaveBreadcrumbAgentD; lpos: the
// world's agents' positions [N][3] in LDS).
__device__ void appendCrumbsD(const DevState &S, int w, uint32_t req, const float *lpos)
{
    if (req == 0) return;
    const int N = S.N;
    const int64_t g0 = (int64_t)w * N;
    float4 *cr = crumbPtr(S, w);
    int n = S.numCrumbs[w];
    int next_id = S.nextCrumbId[w];
    #pragma unroll 1
    for (int i = 0; i < N; i++) {
        const int64_t g = g0 + i;
        if (!(req & (1u << i))) continue;
        if (n < kMaxCrumbs) {
            const int team = i / S.T, off = i - team * S.T;
            cr[2 * n] = make_float4(lpos[3 * i], lpos[3 * i + 1], lpos[3 * i + 2], 1.f);
            cr[2 * n + 1] = make_float4((float)team, (float)off, __int_as_float(next_id), 0.f);
            S.bcLast[g] = next_id;
            next_id += 1;
            n += 1;
        } else {
            S.crumbOverflow[w] += 1;
            S.bcLast[g] = -1;
        }
    }
    S.numCrumbs[w] = n;
    S.nextCrumbId[w] = next_id;
}

// sim.cpp:4892-4926 accumulateBreadcrumbPenaltiesSystem, with its decay and
// compaction of the world's crumbs, by the world's N agent lanes together
// (called by every thread of the block: it has block barriers).  Each round
// the lanes load N consecutive crumbs into LDS (buf: 2 float4 per lane);
// every agent adds the round's crumbs to its penalty in creation order, and
// each lane decays its own crumb and, if it survives, stores it at its
// compacted slot (the survivors before it: earlier rounds' plus this
// round's lower lanes).  Stores only go to slots at or below the round being
// read, whose crumbs are already in LDS.
__device__ __forceinline__ void crumbRoundsD(const DevState &S, int w, int i, bool act, int wl, float4 *buf)
{
    const int N = S.N;
    const int64_t g = (int64_t)w * N + i;
    const int team = i / S.T, off = i - team * S.T;
    float4 *cr = act ? crumbPtr(S, w) : nullptr;
    const int n = act ? S.numCrumbs[w] : 0;
    const Vec3 pos = act ? ldPos(S, g) : v3(0.f, 0.f, 0.f);
    float total = 0.f; // leaveBreadcrumbsSystem's reset (sim.cpp:4845-4889)
    int kept = 0;      // survivors of the earlier rounds
    const float4 *wb = buf + 2 * wl * N;
    // the next round's crumb is loaded while this round runs: it sits at a
    // slot >= r0 + N, which no store of this round (slots < r0 + N) touches
    float4 pn = make_float4(0.f, 0.f, 0.f, 0.f), mn = pn;
    if (i < n) {
        pn = cr[2 * i];
        mn = cr[2 * i + 1];
    }
    #pragma unroll 1
    for (int r0 = 0; __syncthreads_or(r0 < n); r0 += N) {
        const int k = r0 + i;
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f), meta = p;
        if (k < n) {
            p = pn;
            meta = mn;
            buf[2 * threadIdx.x] = p;
            buf[2 * threadIdx.x + 1] = meta;
        }
        if (k + N < n) {
            pn = cr[2 * (k + N)];
            mn = cr[2 * (k + N) + 1];
        }
        __syncthreads();
        if (r0 < n) {
            const int cnt = min(N, n - r0);
            int before = 0, round_kept = 0;
            #pragma unroll 1
            for (int j = 0; j < cnt; j++) {
                const float4 pj = wb[2 * j], mj = wb[2 * j + 1];
                if (!((int)mj.x != team || (int)mj.y == off))
                    if (distance(pos, v3(pj.x, pj.y, pj.z)) <= c::kAgentRadius * 4.f) total += pj.w;
                const bool keep = !(pj.w - 0.025f <= 0.f);
                round_kept += keep ? 1 : 0;
                if (j < i && keep) before += 1;
            }
            if (k < n) {
                p.w -= 0.025f;
                if (!(p.w <= 0.f)) {
                    const int m = kept + before;
                    cr[2 * m] = p;
                    cr[2 * m + 1] = meta;
                }
            }
            kept += round_kept;
        }
    }
    if (act) {
        S.bcPenalty[g] = total;
        if (i == 0) S.numCrumbs[w] = kept;
    }
}

// Filter boxes of updateFiltersState (sim.cpp:128-291): x/y ranges of the
// three hard-coded analytics filters.
__constant__ const int16_t kFiltMinX[3] = { -1272, 852, -32768 }, kFiltMinY[3] = { -866, -851, -32768 };
__constant__ const int16_t kFiltMaxX[3] = { -825, 1280, 32767 }, kFiltMaxY[3] = { 696, 593, 32767 };

__device__ __forceinline__ bool inFilterBoxD(Vec3 p, int fi)
{
    return !(p.x < kFiltMinX[fi] || p.y < kFiltMinY[fi] || p.x > kFiltMaxX[fi] || p.y > kFiltMaxY[fi]);
}

// What zoneMatchInfoSystem + updateFiltersState read per agent, computed by
// the agent's own lane (all in parallel) and handed to the world lane
// through LDS: bit 0 wasKilled, 1 hasDiedDuringEpisode, 2 / 3 inside filter
// box 0 / 1, 4 a landed shot with shooter and target inside filter box 2.
enum : uint32_t { kMbKilled = 1, kMbDied = 2, kMbF0 = 4, kMbF1 = 8, kMbF2 = 16 };

__device__ __forceinline__ uint32_t matchAgentBitsD(const DevState &S, int w, int i)
{
    const int64_t g0 = (int64_t)w * S.N, g = g0 + i;
    const int32_t f = S.flags[g];
    uint32_t b = 0;
    if (f & kFlagWasKilled) b |= kMbKilled;
    if (f & kFlagHasDied) b |= kMbDied;
    const Vec3 p = ldPos(S, g);
    if (inFilterBoxD(p, 0)) b |= kMbF0;
    if (inFilterBoxD(p, 1)) b |= kMbF1;
    const int lo = S.landedOn[g];
    if (lo != -1 && inFilterBoxD(p, 2) && inFilterBoxD(ldPos(S, g0 + lo), 2)) b |= kMbF2;
    return b;
}

// Agent bit masks (bit i = agent i of the world) from the LDS bytes.
struct MatchMasks {
    uint32_t killed, died, f0, f1, f2;
};

__device__ __forceinline__ MatchMasks matchMasksD(const uint8_t *mb, int N)
{
    MatchMasks m = { 0u, 0u, 0u, 0u, 0u };
    #pragma unroll 1
    for (int i = 0; i < N; i++) {
        const uint32_t b = mb[i];
        m.killed |= ((b & kMbKilled) ? 1u : 0u) << i;
        m.died |= ((b & kMbDied) ? 1u : 0u) << i;
        m.f0 |= ((b & kMbF0) ? 1u : 0u) << i;
        m.f1 |= ((b & kMbF1) ? 1u : 0u) << i;
        m.f2 |= ((b & kMbF2) ? 1u : 0u) << i;
    }
    return m;
}

// sim.cpp:128-291 updateFiltersState from the world's agent bits.  The
// filter state is read once (by the caller, with its other loads: last[6]
// [team][filter], act[2]) and written once.
struct FilterState {
    int32_t last[6];
    uint32_t act[2];
};

__device__ __forceinline__ FilterState loadFiltersD(const DevState &S, int w)
{
    FilterState f;
    const int32_t *lastp = &S.filtLast[(int64_t)w * 6];
    for (int k = 0; k < 6; k++) f.last[k] = lastp[k];
    f.act[0] = (uint32_t)S.filtAct0[w];
    f.act[1] = (uint32_t)S.filtAct1[w];
    return f;
}

__device__ __forceinline__ void updateFiltersBitsD(const DevState &S, int w, int cur_step, const MatchMasks &mm,
                                                   FilterState fs)
{
    const int T = S.T;
    int32_t *lastp = &S.filtLast[(int64_t)w * 6]; // [team][filter]
    int32_t *last = fs.last;
    uint32_t *act = fs.act;
    const uint32_t team0 = (1u << T) - 1u, team1 = team0 << T;
    const int min_num[2] = { 5, 1 };
    for (int fi = 0; fi < 3; fi++) {
        for (int t = 0; t < 2; t++) {
            if (act[t] & (1u << fi)) {
                if (cur_step - last[t * 3 + fi] > 0) act[t] &= ~(1u << fi);
            }
        }
        if (fi == 2) {
            // any landed shot inside box 2 activates the shooter's team
            for (int t = 0; t < 2; t++) {
                if (mm.f2 & (t == 0 ? team0 : team1)) {
                    act[t] |= 1u << fi;
                    last[t * 3 + fi] = cur_step;
                }
            }
        } else {
            const uint32_t in = fi == 0 ? mm.f0 : mm.f1;
            const int cnt[2] = { __builtin_popcount(in & team0), __builtin_popcount(in & team1) };
            for (int t = 0; t < 2; t++) {
                if (cnt[t] >= min_num[fi]) {
                    act[t] |= 1u << fi;
                    last[t * 3 + fi] = cur_step;
                }
            }
        }
    }
    for (int k = 0; k < 6; k++) lastp[k] = last[k];
    S.filtAct0[w] = (int32_t)act[0];
    S.filtAct1[w] = (int32_t)act[1];
    if (__builtin_popcount(act[0]) == 3) S.filtMatched0[w] = cur_step;
    if (__builtin_popcount(act[1]) == 3) S.filtMatched1[w] = cur_step;
}

// sim.cpp:4470-4673 zoneMatchInfoSystem
__device__ void writeSnapshotD(const DevState &S, const SceneDev &sc, int w, bool new_captured);

// Run by one lane per world: every world value it reads is loaded up front
// and the results are stored once at the end, so its global accesses are a
// couple of round trips (the agent bytes come from LDS as a char pointer,
// which may alias anything: read-modify-writes through memory next to them
// were reloaded after every LDS read).  The snapshot (events mode) reads
// captured / stepsUntilPoint after this step's update, curStep before it.
__device__ __forceinline__ void zoneMatchInfoD(const DevState &S, const SceneDev &sc, int w, const uint8_t *mb)
{
    const int N = S.N, T = S.T;
    int32_t *mr = &S.matchResult[(int64_t)w * 30];
    int32_t *zs_all = &S.zoneStats[(int64_t)w * 25];
    const MatchMasks mm = matchMasksD(mb, N);
    const int cur_step = S.curStep[w] + 1;
    const int reset_w = S.reset[w];
    int m[5] = { mr[0], mr[1], mr[2], mr[3], mr[4] };
    const int ctrl = S.controlling[w];
    int sup = S.stepsUntilPoint[w];
    bool captured = S.captured[w] != 0;
    const int cz = S.curZone[w];
    const bool contested = S.contested[w] != 0;
    const int team_a = S.teamA[w];
    int32_t *zs = &zs_all[cz * 5];
    int z[5] = { zs[0], zs[1], zs[2], zs[3], zs[4] };
    const FilterState fs = loadFiltersD(S, w); // before this function's stores

    bool finished = cur_step >= c::kEpisodeLen || reset_w == 1;
    if (cur_step == 1) {
        m[0] = -1; m[1] = 0; m[2] = 0; m[3] = 0; m[4] = 0;
    }
    const uint32_t team0 = (1u << T) - 1u, team1 = team0 << T;
    // a killed agent of team t scores for team t ^ 1 (mr[1 + (t ^ 1)])
    m[2] += __builtin_popcount(mm.killed & team0);
    m[1] += __builtin_popcount(mm.killed & team1);
    bool earned = false;
    bool new_captured = false;
    if (sup == 0) {
        sup = c::kZonePointInterval;
        if (!captured) {
            captured = true;
            new_captured = true;
        }
        if (ctrl >= 0) m[3 + ctrl] += 1;
        earned = true;
    }
    if (m[3] >= c::kZoneWinPoints || m[4] >= c::kZoneWinPoints) finished = true;
    // sim.cpp:4534-4575: ZoneCaptureDefend ends on the attacker's first
    // point, the defender's 8th, or when every attacker has died once
    const bool zcd = sc.task == MPENV_TASK_ZONE_CAPTURE_DEFEND;
    const int attacker = team_a == 1 ? 1 : 0, defender = attacker ^ 1;
    bool attackers_all_died = true;
    if (zcd) {
        if (m[3 + attacker] == 1) finished = true;
        if (m[3 + defender] == 8) finished = true;
        const uint32_t am = attacker == 0 ? team0 : team1;
        attackers_all_died = (mm.died & am) == am;
        if (attackers_all_died) finished = true;
    }
    z[4] += 1;
    if (captured && ctrl >= 0) z[1 + ctrl] += 1;
    if (contested) z[3] += 1;
    if (new_captured) z[0] += 1;

    S.stepsUntilPoint[w] = sup;
    S.captured[w] = captured ? 1 : 0;
    S.earned[w] = earned ? 1 : 0;
    for (int k = 0; k < 5; k++) zs[k] = z[k];
    updateFiltersBitsD(S, w, cur_step, mm, fs);
    if (sc.eventsOn) writeSnapshotD(S, sc, w, new_captured);
    if (finished) {
        if (zcd) {
            if (m[3 + attacker] == 1) m[0] = attacker;
            else if (m[3 + defender] == 8 || attackers_all_died) m[0] = defender;
            else m[0] = 2;
        } else if (m[3] > m[4]) m[0] = 0;
        else if (m[4] > m[3]) m[0] = 1;
        else m[0] = 2;
        // every zone's stats in one round of loads, then the stores (one
        // load-store pair per entry waited for each store before the next load)
        int32_t zv[25];
        #pragma unroll
        for (int k = 0; k < 25; k++) zv[k] = zs_all[k];
        #pragma unroll
        for (int k = 0; k < 25; k++) mr[5 + k] = zv[k];
        #pragma unroll
        for (int k = 0; k < 25; k++) zs_all[k] = 0;
    }
    for (int k = 0; k < 5; k++) mr[k] = m[k];
    S.curStep[w] = cur_step;
    S.finished[w] = finished ? 1 : 0;
}

// Capture event + writePackedStepSnapshot (sim.cpp:4592-4634, 41-106).  The
// reference's per-world eventLoggedInStep / eventMask accumulate from every
// logEvent since the last snapshot; here they are folded in from this
// step's event slots, and reset when a snapshot is written (only for a
// valid matchID, i.e. after the first triggered reset).
__device__ void writeSnapshotD(const DevState &S, const SceneDev &sc, int w, bool new_captured)
{
    const int N = S.N;
    const int64_t g0 = (int64_t)w * N;
    const bool valid = S.matchValid[w] != 0;
    if (valid && new_captured) {
        const int cz = S.curZone[w];
        AABB za = sc.tab->zoneAABB[cz];
        Quat to_zone = qinv(angleAxis(sc.tab->zoneRot[cz], kUp));
        za.pMin = rotateVec(to_zone, za.pMin);
        za.pMax = rotateVec(to_zone, za.pMax);
        uint32_t mask = 0;
        const int ctrl = S.controlling[w];
        #pragma unroll 1
        for (int i = 0; i < N; i++) {
            if (i / S.T != ctrl) continue;
            Vec3 p = ldPos(S, g0 + i);
            p.z += c::kStandHeight / 2.f;
            if (aabbContains(za, rotateVec(to_zone, p))) mask |= 1u << i;
        }
        putEventD(S, sc, w, 2 * N, MPENV_EVENT_CAPTURE, cz, ctrl, (int)mask);
    }
    int32_t logged = S.evLogged[w], emask = S.evMask[w];
    const mpenv_game_event *ev = &S.events[(int64_t)w * S.evStride];
    for (int k = 0; k < S.evStride; k++) {
        if (ev[k].type != 0) {
            logged = 1;
            emask |= (int32_t)ev[k].type;
        }
    }
    if (!valid) {
        S.evLogged[w] = logged;
        S.evMask[w] = emask;
        S.snapWritten[w] = 0;
        return;
    }
    mpenv_packed_step_snapshot sn;
    sn.num_events = (uint32_t)logged;
    sn.event_mask = (uint32_t)emask;
    sn.match_id = matchIdD(S, sc, w);
    // the match state and the players as curriculum_core.h packs them (the
    // curriculum pool's k_harvest runs the same lines); curStep is still the
    // value the step began with
    mp::curriculumPackMatch(sn, S.curStep[w], S.curZone[w], S.captured[w], S.controlling[w], S.zoneSteps[w],
                            S.stepsUntilPoint[w]);
    for (int i = 0; i < kMaxAgents; i++) {
        if (i >= N) {
            sn.players[i] = mpenv_packed_player {};
            continue;
        }
        const int64_t g = g0 + i;
        sn.players[i] = mp::curriculumPackPlayer(S.px[g], S.py[g], S.pz[g], S.ayaw[g], S.apitch[g], S.hp[g],
                                                 S.magazine[2 * g], S.magazine[2 * g + 1], S.curPose[g], S.landedOn[g]);
    }
    S.snapshots[w] = sn;
    S.evLogged[w] = 0;
    S.evMask[w] = 0;
    S.snapWritten[w] = 1;
}

// pvpRecordSystem (sim.cpp:4750-4792): per agent lane + curStep by the world lane
__device__ void recordAgentD(const DevState &S, int w, int i)
{
    const int64_t g = (int64_t)w * S.N + i;
    mpenv_agent_log &a = S.recordLog[w].agents[i];
    a.position[0] = S.px[g]; a.position[1] = S.py[g]; a.position[2] = S.pz[g];
    a.aim_yaw = S.ayaw[g];
    a.aim_pitch = S.apitch[g];
    a.aim_rot[0] = S.aw[g]; a.aim_rot[1] = S.ax[g]; a.aim_rot[2] = S.ay[g]; a.aim_rot[3] = S.az[g];
    a.hp = S.hp[g];
    a.mag_num_bullets = S.magazine[2 * g];
    a.mag_is_reloading = S.magazine[2 * g + 1];
    a.cur_pose = S.curPose[g];
    a.tgt_pose = S.tgtPose[g];
    a.transition_remaining = S.transRem[g];
    a.shot_agent_idx = S.landedOn[g];
    a.fired_shot_t = S.firedT[g];
    a.was_killed = (S.flags[g] & kFlagWasKilled) ? 1 : 0;
    a.successful_kill = (S.flags[g] & kFlagSuccessfulKill) ? 1 : 0;
    a.pad_[0] = 0;
    a.pad_[1] = 0;
}

// pvpReplaySystem (sim.cpp:4794-4843) for one agent (shot visualisation,
// viewer-only, is skipped)
__device__ void replayAgentD(const DevState &S, int w, int i)
{
    const int64_t g = (int64_t)w * S.N + i;
    const mpenv_agent_log &a = S.replayLog[w].agents[i];
    S.px[g] = a.position[0]; S.py[g] = a.position[1]; S.pz[g] = a.position[2];
    S.ayaw[g] = a.aim_yaw;
    S.apitch[g] = a.aim_pitch;
    S.aw[g] = a.aim_rot[0]; S.ax[g] = a.aim_rot[1]; S.ay[g] = a.aim_rot[2]; S.az[g] = a.aim_rot[3];
    stRot(S, g, qnormalize(angleAxis(a.aim_yaw, kUp)));
    S.hp[g] = a.hp;
    S.magazine[2 * g] = a.mag_num_bullets;
    S.magazine[2 * g + 1] = a.mag_is_reloading;
    S.curPose[g] = a.cur_pose;
    S.tgtPose[g] = a.tgt_pose;
    S.transRem[g] = a.transition_remaining;
    S.landedOn[g] = a.shot_agent_idx;
    S.firedT[g] = a.fired_shot_t;
    int32_t fl = S.flags[g] & ~(kFlagWasKilled | kFlagSuccessfulKill);
    if (a.was_killed) fl |= kFlagWasKilled | kFlagHasDied;
    if (a.successful_kill) fl |= kFlagSuccessfulKill;
    S.flags[g] = fl;
}

// sim.cpp:3998-4087 distToZOBB + evaluateGoalRegionsSystem
// distToZOBB (sim.cpp:3998-4020) with the frame precomputed (k_scene_frames)
__device__ __forceinline__ float distToFrameD(const FrameDev &f, Vec3 pos)
{
    const Vec3 p = rotateVec(f.toFrame, pos);
    float sq = 0.f;
    for (int i = 0; i < 3; i++) {
        float v = comp(p, i);
        if (v < comp(f.pMin, i)) { float d = comp(f.pMin, i) - v; sq += d * d; }
        if (v > comp(f.pMax, i)) { float d = v - comp(f.pMax, i); sq += d * d; }
    }
    return sqrt_(sq);
}

// Agent lanes: the agent's distance to each sub-region of the goals its team
// is scored on (the world lane's inner loop, spread over the agents);
// d[r * 3 + s], unused entries left alone.
__device__ __forceinline__ void goalDistAgentD(const DevState &S, const SceneDev &sc, int w, int i, Vec3 pos, float *d)
{
    const int attacker = S.teamA[w];
    const int team = i / S.T;
    for (int r = 0; r < sc.numGoals && r < 2; r++) {
        const GoalRegionDev &gr = sc.tab->goals[r];
        const int region_team = gr.attackerTeam ? attacker : (attacker ^ 1);
        if (team != region_team) continue;
        for (int s = 0; s < gr.numSub; s++) d[r * 3 + s] = distToFrameD(sc.tab->goalFrame[r][s], pos);
    }
}

// gd: the world's agents' goalDistAgentD rows in LDS (stride 6).
__device__ __forceinline__ void goalRegionsD(const DevState &S, const SceneDev &sc, int w, const float *gd)
{
    const int N = S.N;
    float team_step[2] = { 0.f, 0.f };
    float mins[2] = { S.goalMin0[w], S.goalMin1[w] };
    const int attacker = S.teamA[w];
    for (int r = 0; r < sc.numGoals && r < 2; r++) {
        const GoalRegionDev &gr = sc.tab->goals[r];
        const int region_team = gr.attackerTeam ? attacker : (attacker ^ 1);
        float max_min = -kFltMax;
        for (int s = 0; s < gr.numSub; s++) {
            float min_d = kFltMax;
            #pragma unroll 1
            for (int i = 0; i < N; i++) {
                if (i / S.T != region_team) continue;
                float d = gd[i * 6 + r * 3 + s];
                if (d < min_d) min_d = d;
            }
            if (min_d > max_min) max_min = min_d;
        }
        float prev = mins[r];
        if (prev == kFltMax) {
            mins[r] = max_min;
        } else {
            float diff = prev - max_min;
            if (diff > 0.f) {
                mins[r] = max_min;
                team_step[region_team] += diff * gr.rewardStrength;
            }
        }
    }
    S.goalMin0[w] = mins[0];
    S.goalMin1[w] = mins[1];
    S.goalTeam0[w] = team_step[0];
    S.goalTeam1[w] = team_step[1];
}

// sim.cpp:3508-3536 exploreVisitedSystem.  The reference keeps a u32
// episode tag per cell and counts a cell when its tag differs from the
// current episode index, then stores the index.  Tags only ever take the
// current, increasing index (curEpisodeIdx = worldEpisodeCounter++), so
// "tag == current episode" is all the state that matters: one bit per cell
// for the agent's episode exploreEp, cleared when the episode moves on
// (lazily, here).  Episode 0 starts from level_gen.cpp:166-171's tags: 0 on
// cells outside the y<40, x<40 quadrant, i.e. already set (k_init_explore).
// Bits live in 8 x 8-cell u64 tiles; the current tile is cached in SoA
// columns and written back to the row when the agent leaves it.

__device__ void exploreVisitedD(const DevState &S, int w, int64_t g)
{
    Vec3 delta = ldPos(S, g) - v3(S.sx[g], S.sy[g], S.sz[g]);
    int32_t x = f2iSatD((delta.x + 0.5f) / (c::kAgentRadius * 2.f));
    int32_t y = f2iSatD((delta.y + 0.5f) / (c::kAgentRadius * 2.f));
    int64_t cx = (int64_t)x + c::kGridMax, cy = (int64_t)y + c::kGridMax;
    if (cx < 0 || cx >= kGridW || cy < 0 || cy >= kGridW) return;
    uint64_t *row = &S.exploreBits[g * kExploreTiles];
    const int32_t cur = S.episode[w];
    int32_t tile = S.exploreTile[g];
    uint64_t word = (uint64_t)(uint32_t)S.exploreLo[g] | ((uint64_t)(uint32_t)S.exploreHi[g] << 32);
    if (S.exploreEp[g] != cur) {
        for (int k = 0; k < kExploreTiles; k++) row[k] = 0ull;
        S.exploreEp[g] = cur;
        tile = -1;
    }
    const int t = exploreTileD((int)cx, (int)cy);
    if (t != tile) {
        if (tile >= 0) row[tile] = word;
        word = row[t];
        tile = t;
        S.exploreTile[g] = t;
    }
    const uint64_t bit = 1ull << exploreBitD((int)cx, (int)cy);
    if (!(word & bit)) {
        word |= bit;
        if (length2(delta) > 2.f) S.newCells[g] += 1;
    }
    S.exploreLo[g] = (int32_t)(uint32_t)word;
    S.exploreHi[g] = (int32_t)(uint32_t)(word >> 32);
}

// sim.cpp:4089-4200 zoneCaptureDefendRewardSystem: goal-region progress,
// kills and control of the zone by the agent's own team, +-20 / -5 at the
// end of the match; no curriculum, breadcrumb or area terms.
__device__ float zoneCaptureDefendRewardD(const DevState &S, const SceneDev &sc, int w, int i)
{
    const int64_t g = (int64_t)w * S.N + i;
    const int team = i / S.T;
    int32_t flags = S.flags[g];
    const float *rc = &S.rewardCoefs[9 * g];
    const float shot = rc[1], explore = rc[2], ctrl_s = rc[5], earned_s = rc[7];
    float r = 0.f;
    r += 0.02f * (team == 0 ? S.goalTeam0[w] : S.goalTeam1[w]);
    if (flags & kFlagReloadedFullMag) r -= 0.01f;
    if (flags & kFlagSuccessfulKill) r += 1.f;
    if (S.landedOn[g] != -1) r += shot * 1.f;
    if (flags & kFlagWasKilled) r -= 1.f;
    if (S.wasShot[g] > 0) r -= shot * 1.f;
    uint32_t nn = (uint32_t)S.newCells[g];
    S.newCells[g] = 0;
    if (nn > 0) r += float(nn) * explore;
    if (!(flags & kFlagInZone)) {
        AABB za = sc.tab->zoneAABB[S.curZone[w]];
        Vec3 center = (za.pMax + za.pMin) / 2.f;
        float dist = distance(center, ldPos(S, g));
        if (dist < S.minDistZone[g]) S.minDistZone[g] = dist;
    }
    const int ctrl = S.controlling[w];
    if (ctrl != -1 && ctrl == team) {
        r += ctrl_s;
        if (S.earned[w]) r += earned_s;
    }
    if (S.finished[w]) {
        const int win = S.matchResult[(int64_t)w * 30];
        if (win == 2) r -= 5.f;
        else if (win == team) r += 20.f;
        else r -= 20.f;
    }
    if (S.alive[g] == 0.f) {
        S.flags[g] = flags & ~(kFlagSuccessfulKill | kFlagWasKilled);
        S.landedOn[g] = -1;
        S.wasShot[g] = 0;
        S.firedT[g] = -kFltMax;
    }
    S.reward[g] = r;
    return r;
}

// sim.cpp:3734-3847 subzoneRewardSystem (after the LearnShooting branch,
// which zoneRewardD handles for both): kills pay 3, the agent's own
// sub-zone drives the in-zone / approach / control terms, no earned-point
// or area terms.
__device__ float subzoneRewardD(const DevState &S, const SceneDev &sc, int w, int i)
{
    const int64_t g = (int64_t)w * S.N + i;
    int32_t flags = S.flags[g];
    const int landed = S.landedOn[g];
    const float *rc = &S.rewardCoefs[9 * g];
    const float shot = rc[1], explore = rc[2], in_zone = rc[3], ctrl_s = rc[5], zdist = rc[6], crumb = rc[8];
    float r = 0.f;
    r -= crumb * S.bcPenalty[g];
    if (flags & kFlagReloadedFullMag) r -= 0.5f;
    if (flags & kFlagSuccessfulKill) r += 3.f;
    if (landed != -1) r += shot * 1.f;
    if (flags & kFlagWasKilled) r -= 1.5f;
    if (S.wasShot[g] > 0) r -= shot * 1.f;
    uint32_t nn = (uint32_t)S.newCells[g];
    S.newCells[g] = 0;
    if (nn > 0) r += float(nn) * explore;
    const int k = subZoneIndexD(S, g);
    if (flags & kFlagInSubZone) {
        r += in_zone;
    } else {
        const ZOBBDev &sz = sc.tab->subZones[k];
        Vec3 center = (sz.pMax + sz.pMin) / 2.f;
        float dist = distance(center, ldPos(S, g));
        float md = S.minDistSub[g];
        if (dist < md) {
            float scale = zdist;
            if (!(flags & kFlagHasDied)) scale *= 10.f;
            r += scale * (md - dist);
            S.minDistSub[g] = dist;
        }
    }
    const int ctrl = subCtrlD((uint32_t)S.subState[w], k);
    if (ctrl != -1) {
        if (ctrl == i / S.T) r += ctrl_s;
        else r -= ctrl_s;
    }
    if (S.alive[g] == 0.f) {
        S.flags[g] = flags & ~(kFlagSuccessfulKill | kFlagWasKilled);
        S.landedOn[g] = -1;
        S.wasShot[g] = 0;
        S.firedT[g] = -kFltMax;
    }
    S.reward[g] = r;
    return r;
}

// sim.cpp:3849-3996 zoneRewardSystem (+ learnShootingRewardSystem 3707-3732)
// Every reward system returns the reward it stored (k_sim hands it to the
// team reward through LDS).
__device__ __forceinline__ float zoneRewardD(const DevState &S, const SceneDev &sc, int w, int i)
{
    const int64_t g0 = (int64_t)w * S.N;
    const int64_t g = g0 + i;
    int32_t flags = S.flags[g];
    const int landed = S.landedOn[g];
    float r = 0.f;
    if (sc.task == MPENV_TASK_ZONE_CAPTURE_DEFEND) {
        return zoneCaptureDefendRewardD(S, sc, w, i);
    }
    if (S.worldCurr[w] == 0) {
        if (landed != -1) r += 0.5f;
        else if (S.firedT[g] >= 0.f) r -= 0.05f;
        if (flags & kFlagReloadedFullMag) r -= 0.5f;
        S.reward[g] = r;
        return r;
    }
    if (sc.simFlags & kFlagSubZones) {
        return subzoneRewardD(S, sc, w, i);
    }
    const float *rc = &S.rewardCoefs[9 * g];
    const float shot = rc[1], explore = rc[2], in_zone = rc[3], ctrl_s = rc[5], zdist = rc[6], earned_s = rc[7],
                crumb = rc[8];
    const int team = i / S.T, off = i - team * S.T;
    const Vec3 pos = ldPos(S, g);
    r -= crumb * S.bcPenalty[g];
    if (flags & kFlagReloadedFullMag) r -= 0.5f;
    if (flags & kFlagSuccessfulKill) r += 1.f;
    if (landed != -1) r += shot * 1.f;
    if (flags & kFlagWasKilled) r -= 1.5f;
    if (S.wasShot[g] > 0) r -= shot * 1.f;
    uint32_t nn = (uint32_t)S.newCells[g];
    S.newCells[g] = 0;
    if (nn > 0) r += float(nn) * explore;
    if (flags & kFlagInZone) {
        r += in_zone;
    } else {
        AABB za = sc.tab->zoneAABB[S.curZone[w]];
        Vec3 center = (za.pMax + za.pMin) / 2.f;
        float dist = distance(center, pos);
        float md = S.minDistZone[g];
        if (dist < md) {
            float scale = zdist;
            if (!(flags & kFlagHasDied)) scale *= 10.f;
            r += scale * (md - dist);
            S.minDistZone[g] = dist;
        }
    }
    const int ctrl = S.controlling[w];
    const bool earned = S.earned[w] != 0;
    if (ctrl != -1) {
        if (ctrl == team) {
            r += ctrl_s;
            if (earned) r += earned_s;
        } else {
            r -= ctrl_s;
            if (earned) r -= earned_s;
        }
    }
    if (S.alive[g] == 0.f) {
        S.flags[g] = flags & ~(kFlagSuccessfulKill | kFlagWasKilled);
        S.landedOn[g] = -1;
        S.wasShot[g] = 0;
        S.firedT[g] = -kFltMax;
        S.reward[g] = r;
        return r;
    }
    {
        float poly = 0.f;
        const int num_teammates = S.T - 1;
        for (int k = 0; k < num_teammates - 1; k++) {
            const int64_t t1 = g0 + team * S.T + (k < off ? k : k + 1);
            const int64_t t2 = g0 + team * S.T + (k + 1 < off ? k + 1 : k + 2);
            float e1x = S.px[t1] - pos.x, e1y = S.py[t1] - pos.y;
            float e2x = S.px[t2] - pos.x, e2y = S.py[t2] - pos.y;
            float tri = e1x * e2y - e1y * e2x;
            poly += fabs_(tri);
        }
        float dx = sc.worldBounds.pMax.x - sc.worldBounds.pMin.x;
        float dy = sc.worldBounds.pMax.y - sc.worldBounds.pMin.y;
        float area = dx * dy;
        float frac = poly / (2.f * area);
        r += frac * 1e-2f;
    }
    S.reward[g] = r;
    return r;
}

// ====================================================== kernels

// Persistent-entity setup + the Sim constructor's initWorld(ctx, true)
// (sim.cpp:5850-5980, level_gen.cpp:19-328).  One thread per world.
__global__ void __launch_bounds__(64) k_construct(DevState S, SceneDev sc, int32_t tc0, int32_t tc1, int32_t tc2)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= S.W) return;
    const int N = S.N;
    const int64_t g0 = (int64_t)w * N;
    #pragma unroll 1
    for (int i = 0; i < N; i++) {
        const int64_t g = g0 + i;
        S.policy[g] = 0;
        S.aimAction[2 * g] = 0.f; S.aimAction[2 * g + 1] = 0.f;
        S.discreteAim[2 * g] = c::kDiscreteAimYawBuckets / 2;
        S.discreteAim[2 * g + 1] = c::kDiscreteAimPitchBuckets / 2;
        S.dyv[g] = 0.f; S.dpv[g] = 0.f;
        for (int k = 0; k < kMaxTeamSize; k++) S.dmg[(int64_t)k * S.dmgStride + g] = 0.f;
        stRot(S, g, quat(1, 0, 0, 0));
        stAimRot(S, g, quat(1, 0, 0, 0));
        S.landedOn[g] = -1;
        S.bcLast[g] = -1;
        S.flags[g] = 0;
    }
    S.episode[w] = 0;
    S.episodeCounter[w] = 0;
    S.curTier[w] = 0;
    S.curSpawnIdx[w] = 0;
    S.numCrumbs[w] = 0;
    S.nextCrumbId[w] = 0;
    S.crumbOverflow[w] = 0;
    S.reset[w] = 0;
    for (int k = 0; k < 6; k++) S.filtLast[(int64_t)w * 6 + k] = 0;
    S.worldCurr[w] = 1; // WorldCurriculum::FullMatch (sim.cpp:5959)
    const int32_t tc[3] = { tc0, tc1, tc2 };
    initWorldD(S, sc, w, true, tc, MemAgents{ S, g0, sc.aSpawns, sc.bSpawns, sc.commonRespawns }, DrawnKeys{}, SpawnApply{});
    S.matchValid[w] = 0; // matchID = ~0 after construction (sim.cpp:5971)
    S.evLogged[w] = 0;
    S.evMask[w] = 0;
    S.snapWritten[w] = 0;
    for (int k = 0; k < 25; k++) S.zoneStats[(int64_t)w * 25 + k] = 0;
    S.filtAct0[w] = 0; S.filtAct1[w] = 0;
    S.filtMatched0[w] = -1; S.filtMatched1[w] = -1;
}

// ExploreTracker initial contents (level_gen.cpp:166-171: 0xFFFFFFFF on the
// y<40, x<40 quadrant; the other cells start at 0) as the
// bitset of episode 0: the cells whose tag is 0 are set; no tile cached.
__global__ void __launch_bounds__(256) k_init_explore(DevState S, int64_t total)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (int64_t)gridDim.x * blockDim.x) {
        const int t = (int)(k % kExploreTiles);
        const int tx = t % kExploreTilesX, ty = t / kExploreTilesX;
        uint64_t v = 0ull;
        for (int b = 0; b < 64; b++) {
            const int x = tx * 8 + (b & 7), y = ty * 8 + (b >> 3);
            if (x >= kGridW || y >= kGridW) continue;
            if (!(y < c::kGridMax && x < c::kGridMax)) v |= 1ull << b;
        }
        S.exploreBits[k] = v;
        if (t == 0) {
            const int64_t g = k / kExploreTiles;
            S.exploreEp[g] = 0;
            S.exploreTile[g] = -1;
            S.exploreLo[g] = 0;
            S.exploreHi[g] = 0;
        }
    }
}

__global__ void __launch_bounds__(64) k_reset_only(DevState S, SceneDev sc)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= S.W) return;
    resetSystemD(S, sc, w, MemAgents{ S, (int64_t)w * S.N, sc.aSpawns, sc.bSpawns, sc.commonRespawns }, DrawnKeys{}, SpawnApply{});
}

// The Step graph up to and including resetSystem, one workgroup per tile of
// floor(256 / N) worlds, one lane per agent.
// Step graph part 2 (fireSystem onward): per-world phases.  A workgroup
// holds floor(kSimBlock / N) whole worlds, lane = agent, phases separated
// by workgroup barriers.
constexpr int kSimBlock = 128;
// k_sim's dynamic LDS: the BVH image, then the spawn lists.  The phases
// after the last BVH use reuse the image's bytes: the reset's draw keys
// (kPreDraws + 1 per lane) from its start, the spawn records (kSpawnRec
// floats per lane) behind them, and respawnCoopD's scratch (4 floats per
// lane) in the keys' place, which the reset fills only later.
constexpr size_t kSimKeyBytes = (size_t)kSimBlock * (kPreDraws + 1) * sizeof(RandKey);
constexpr size_t kSimRecOffset = kSimKeyBytes;
constexpr size_t kSimRecBytes = (size_t)kSimBlock * kSpawnRec * sizeof(float);
constexpr size_t kSimCoopBytes = (size_t)kSimBlock * 4 * sizeof(float);
constexpr size_t kSimReuseBytes = kSimRecOffset + kSimRecBytes;
static_assert(kSimCoopBytes <= kSimRecOffset, "respawnCoopD's scratch must end below the spawn records");
static_assert(kSimReuseBytes == kSimKeyBytes + kSimRecBytes, "the keys and the records are all that reuses the BVH image");
// (kStaged: the image is in LDS; otherwise only the reused bytes are there)
template <bool kStaged>
__host__ __device__ size_t simSpawnOffset(const SceneDev &sc)
{
    const size_t bvh = kStaged ? CollisionImage { sc.numNodes, sc.numVerts }.bytes() : 0;
    return ((bvh > kSimReuseBytes ? bvh : kSimReuseBytes) + 15) & ~(size_t)15;
}

// k_sim's per-agent floats for the world lane (static LDS), one struct per
// phase in one union: a phase's writes begin after the barrier that ends the
// previous phase's reads.  Integers are stored as float bits.
struct SimFireLds { float px[kSimBlock], py[kSimBlock], pz[kSimBlock], hp[kSimBlock], respawn[kSimBlock]; };
// (also the crumbs' positions in pos and the reset's flags in flags)
struct SimRespawnLds { float pos[3 * kSimBlock], flags[kSimBlock]; };
struct SimCrumbLds { float4 buf[2 * kSimBlock]; };
struct SimGoalLds { float dist[6 * kSimBlock]; };
// (team: 2 per world, at most kSimBlock / 2 worlds as N >= 2)
struct SimRewardLds { float rew[kSimBlock], team[kSimBlock]; };
union SimLds {
    SimFireLds fire;
    SimRespawnLds respawn;
    SimCrumbLds crumb;
    SimGoalLds goal;
    SimRewardLds reward;
};
static_assert(sizeof(SimFireLds) <= sizeof(SimLds) && sizeof(SimRespawnLds) <= sizeof(SimLds) &&
                  sizeof(SimCrumbLds) <= sizeof(SimLds) && sizeof(SimGoalLds) <= sizeof(SimLds) &&
                  sizeof(SimRewardLds) <= sizeof(SimLds),
              "every phase fits the union");
static_assert(sizeof(SimLds) == (size_t)kSimBlock * 8 * sizeof(float), "k_sim's static LDS stays at 8 floats per lane");
// the reset's flags are written while the world lanes still read the rewards
static_assert(offsetof(SimRespawnLds, flags) >= sizeof(SimRewardLds), "reset flags must not overlap the rewards");

template <class LBVH>
__device__ __forceinline__ float flankRewardD(const DevState &S, const SceneDev &sc, const LBVH &bvh, int w, int i);

// 4 waves/SIMD (128 VGPRs, at the price of ~420 B/lane of scratch spills):
// k_sim alone 0.196 -> 0.139 ms -- every wave of a C3 launch resident,
// which hides the per-world phases' latency better than the spills cost.
#define MP_SIM_ATTR __attribute__((amdgpu_waves_per_eu(4)))
// flatten: every phase inlined (an outlined call needs a stack frame in
// scratch for the whole kernel and spills around the call).
template <class LBVH>
__device__ __forceinline__ __attribute__((flatten)) void simBody(const DevState &S, const SceneDev &sc, char *img)
{

    extern __shared__ __attribute__((aligned(16))) char smem[];
    // dynamic LDS (simLdsBytes): the BVH image, which the reset phase reuses
    // for its draw keys, then the scene's spawn lists
    Spawn *const tabA = reinterpret_cast<Spawn *>(smem + simSpawnOffset<LBVH::kStaged>(sc));
    Spawn *const tabB = tabA + sc.numA, *const tabC = tabB + sc.numB;
    {
        const int nq = (sc.numA + sc.numB + sc.numCommon) * (int)(sizeof(Spawn) / 16);
        const int na = sc.numA * (int)(sizeof(Spawn) / 16), nb = sc.numB * (int)(sizeof(Spawn) / 16);
        uint4 *dst = reinterpret_cast<uint4 *>(tabA);
        for (int k = threadIdx.x; k < nq; k += blockDim.x) {
            const uint4 *src = k < na ? reinterpret_cast<const uint4 *>(sc.aSpawns) + k
                             : k < na + nb ? reinterpret_cast<const uint4 *>(sc.bSpawns) + (k - na)
                                           : reinterpret_cast<const uint4 *>(sc.commonRespawns) + (k - na - nb);
            dst[k] = *src;
        }
    }
    const LBVH bvh = stageBVH<LBVH>(LBVH::kStaged ? smem : img, sc); // (its barrier also covers the spawn lists)
    // spawn records in the BVH's LDS once nothing reads the BVH any more:
    // the respawn (after fireD) unless the flank reward traces rays later,
    // the reset (last phase) unless curriculum snapshots rewrite agents after
    // the spawn (then the world lane stores everything itself)
    float *const spawnRec = reinterpret_cast<float *>(smem + kSimRecOffset);
    const bool recRespawn = !sc.flank && !(sc.simFlags & kFlagNoRespawn);
    const bool recReset = sc.numSnapshots == 0;
    const int N = S.N;
    const int wpb = kSimBlock / N;
    const int wl = threadIdx.x / N;
    const int i = threadIdx.x - wl * N;
    const int w = (int)xcdBlockId() * wpb + wl;
    const bool act = (wl < wpb) && (w < S.W);
    const bool wlane = act && i == 0;
    const int64_t g = (int64_t)w * N + i;

    __shared__ uint8_t agentB[kSimBlock]; // per-agent bytes for the world lane (alive, done)
    __shared__ SimLds lds;
    float *const sposL = lds.respawn.pos;
    float *const sflagL = lds.respawn.flags;
    // my world's agents in LDS for the world lane's respawn and reset (which
    // reads only the flags, resetPreD's by then, and the lists)
    const LdsAgents worldL = { &sposL[3 * wl * N], &agentB[wl * N], &sflagL[wl * N], tabA, tabB, tabC };
    if (act && sc.eventsOn) { // ClearTmpNode<GameEventEntity> at step start (sim.cpp:5344)
        mpenv_game_event *ev = &S.events[(int64_t)w * S.evStride];
        ev[2 * i].type = 0;
        ev[2 * i + 1].type = 0;
        if (wlane) ev[2 * N].type = 0;
    }
    if (sc.replayOn) {
        // pvpReplayLogic: pvpReplaySystem then zoneSystem
        if (act) replayAgentD(S, w, i);
        if (wlane) S.curStep[w] = S.replayLog[w].cur_step;
        __syncthreads();
        if (wlane) zoneSystemD(S, sc, w);
        __syncthreads();
    } else {
        {
            // every agent's own fire inputs in one round of loads; the
            // world's positions, hp and respawn counters (the shots' capsule
            // tests and targets) through LDS
            SimFireLds &f = lds.fire;
            FireIn fin;
            if (act) {
                fin = fireLoadD(S, g);
                f.px[threadIdx.x] = fin.pos.x;
                f.py[threadIdx.x] = fin.pos.y;
                f.pz[threadIdx.x] = fin.pos.z;
                f.hp[threadIdx.x] = fin.hp;
                f.respawn[threadIdx.x] = __int_as_float(fin.respawn);
            }
            __syncthreads();
            if (act) fireD(S, sc, bvh, w, i, fin, f.px, f.py, f.pz, f.hp, f.respawn, wl * N);
        }
        __syncthreads();
        // the agents' alive states, positions and flags go to the world
        // lane's respawn through LDS (it read them back from memory one
        // agent at a time)
        bool dead_now = false;
        if (act) {
            const DmgOut d = applyDmgD(S, g);
            dead_now = !d.alive;
            agentB[threadIdx.x] = d.alive ? 1 : 0;
            sposL[3 * threadIdx.x] = d.pos.x;
            sposL[3 * threadIdx.x + 1] = d.pos.y;
            sposL[3 * threadIdx.x + 2] = d.pos.z;
            sflagL[threadIdx.x] = __int_as_float(d.flags);
        }
        __syncthreads();
        const bool coopRespawn = recRespawn && sc.numCommon > 0 && sc.numCommon <= 64 &&
                                 !(sc.simFlags & kFlagNavmeshSpawn);
        if (coopRespawn)
            respawnCoopD(S, sc, w, i, wl, act, worldL, spawnRec + wl * N * kSpawnRec, reinterpret_cast<float *>(smem));
        else if (wlane && !(sc.simFlags & kFlagNoRespawn)) {
            if (recRespawn) respawnSerialD(S, sc, w, worldL, SpawnRecord{ spawnRec + wl * N * kSpawnRec });
            else respawnSerialD(S, sc, w, worldL, SpawnApply{});
        }
        if (recRespawn) {
            // the respawned agents' own stores, from the world lane's records
            __syncthreads();
            if (dead_now) {
                const ZoneBox zb = zoneBoxD(sc, S.curZone[w]);
                spawnApplyD(S, sc, g, true, ldSpawnRecD(spawnRec + threadIdx.x * kSpawnRec), __float_as_int(sflagL[threadIdx.x]), zb);
            }
        }
        __syncthreads();
        {
            __shared__ int zoneCz[kSimBlock];
            __shared__ uint8_t zoneIn[kSimBlock];
            ZonePre zp;
            if (wlane) {
                zp = zonePreD(S, sc, w);
                zoneCz[wl] = zp.cz;
            }
            __syncthreads();
            // Agent phase shared by the zone test, the recorder and
            // leaveBreadcrumbs: none reads what another writes (InZone and
            // CrumbRequest are different flag bits of the lane's own agent;
            // the recorder reads neither), so they run between one pair of
            // barriers instead of three.
            if (act) {
                // bit 0 in the zone, bit 1 a new breadcrumb requested
                const bool zin = zoneInD(S, sc, zoneCz[wl], g);
                if (sc.recordOn) recordAgentD(S, w, i);
                const bool req = leaveBreadcrumbAgentD(S, w, g);
                zoneIn[threadIdx.x] = (zin ? 1 : 0) | (req ? 2 : 0);
                // the position a requested crumb takes
                const Vec3 p = ldPos(S, g);
                sposL[3 * threadIdx.x] = p.x;
                sposL[3 * threadIdx.x + 1] = p.y;
                sposL[3 * threadIdx.x + 2] = p.z;
            }
            if (wlane && sc.recordOn) S.recordLog[w].cur_step = S.curStep[w];
            __syncthreads();
            if (wlane) {
                int na = 0, nb = 0;
                uint32_t req = 0;
                #pragma unroll 1
                for (int k = 0; k < N; k++) {
                    const int b = zoneIn[wl * N + k];
                    if (b & 2) req |= 1u << k;
                    if (!(b & 1)) continue;
                    if (k / S.T == 0) na += 1;
                    else nb += 1;
                }
                zonePostD(S, w, zp, na, nb);
                if (sc.simFlags & kFlagSubZones) subzoneSystemD(S, sc, w);
                appendCrumbsD(S, w, req, &sposL[3 * wl * N]);
            }
        }
        __syncthreads();
        // accumulateBreadcrumbPenalties and the crumbs' decay (the end of
        // that system), in rounds over LDS
        crumbRoundsD(S, w, i, act, wl, lds.crumb.buf);
    }
    // zoneMatchInfoSystem's per-agent reads, one lane per agent (the world
    // lane would otherwise walk them serially)
    __shared__ uint8_t matchBits[kSimBlock];
    if (act) {
        matchBits[threadIdx.x] = (uint8_t)matchAgentBitsD(S, w, i);
        goalDistAgentD(S, sc, w, i, ldPos(S, g), &lds.goal.dist[threadIdx.x * 6]);
    }
    __syncthreads();
    if (wlane) {
        zoneMatchInfoD(S, sc, w, &matchBits[wl * N]);
        goalRegionsD(S, sc, w, &lds.goal.dist[wl * N * 6]);
    }
    __syncthreads();
    // rewards and done flags go to the world lane through LDS (rewL, agentB)
    // instead of being read back from memory one agent at a time
    float *const rewL = lds.reward.rew;
    float *const teamL = lds.reward.team;
    if (act) {
        exploreVisitedD(S, w, g);
        if (sc.flank && sc.task == MPENV_TASK_ZONE) rewL[threadIdx.x] = flankRewardD(S, sc, bvh, w, i);
        else rewL[threadIdx.x] = zoneRewardD(S, sc, w, i);
    }
    __syncthreads();
    if (wlane) {
        // pvpTeamRewardSystem (sim.cpp:4292-4313)
        float tr[2] = { 0.f, 0.f };
        int ts[2] = { 0, 0 };
        #pragma unroll 1
        for (int j = 0; j < N; j++) {
            int t = j / S.T;
            tr[t] += rewL[wl * N + j];
            ts[t] += 1;
        }
        tr[0] /= float(ts[0]);
        tr[1] /= float(ts[1]);
        S.teamRew0[w] = tr[0];
        S.teamRew1[w] = tr[1];
        teamL[2 * wl] = tr[0];
        teamL[2 * wl + 1] = tr[1];
    }
    __syncthreads();
    if (act) {
        // pvpFinalRewardSystem (sim.cpp:4315-4339) + doneSystem (4712-4717)
        const int team = i / S.T;
        const float spirit = S.rewardCoefs[9 * g];
        const bool done = S.finished[w] != 0;
        const float my = rewL[threadIdx.x];
        const float team_r = teamL[2 * wl + team];
        const float fr = my * (1.f - spirit) + team_r * spirit;
        S.reward[g] = fr;
        S.done[g] = done ? 1 : 0;
        rewL[threadIdx.x] = fr;
        agentB[threadIdx.x] = done ? 1 : 0;
    }
    // resets: the agents' own parts in parallel, then the world lane
    // (the BVH image is dead from here on: the reset's draw keys go there)
    RandKey *pre = reinterpret_cast<RandKey *>(smem) + (int64_t)wl * N * (kPreDraws + 1);
    const bool resetting = act && resetDueD(S, sc, w);
    if (resetting) sflagL[threadIdx.x] = __int_as_float(resetPreD(S, sc, w, i, pre + i * (kPreDraws + 1)));
    __syncthreads();
    if (wlane) {
        // fullTeamDoneRewardSystem (sim.cpp:4720-4747)
        for (int t = 0; t < 2; t++) {
            float r = 0.f;
            bool done = true;
            for (int j = t * S.T; j < (t + 1) * S.T; j++) {
                r += rewL[wl * N + j];
                if (!agentB[wl * N + j]) done = false;
            }
            S.ftReward[(int64_t)w * 2 + t] = r;
            S.ftDone[(int64_t)w * 2 + t] = done ? 1 : 0;
        }
        if (recReset) resetSystemD(S, sc, w, worldL, PreparedKeys{ pre }, SpawnRecord{ spawnRec + wl * N * kSpawnRec });
        else resetSystemD(S, sc, w, worldL, PreparedKeys{ pre }, SpawnApply{});
    }
    if (recReset) {
        // the reset agents' own stores, from the world lane's records
        __syncthreads();
        if (resetting) {
            const ZoneBox zb = zoneBoxD(sc, S.curZone[w]);
            spawnApplyD(S, sc, g, false, ldSpawnRecD(spawnRec + threadIdx.x * kSpawnRec), __float_as_int(sflagL[threadIdx.x]), zb);
            resetAgentTailD(S, g);
        }
    }
}

__global__ void __launch_bounds__(kSimBlock) MP_SIM_ATTR __attribute__((flatten)) k_sim(DevState S, SceneDev sc)
{
    simBody<LBVHL>(S, sc, nullptr);
}

__global__ void __launch_bounds__(kSimBlock) MP_SIM_ATTR __attribute__((flatten)) k_sim_g(DevState S, SceneDev sc, SceneImages img)
{
    simBody<LBVHG>(S, sc, img.sphere);
}

// sim.cpp:4202-4278 flankRewardSystem (Task.Zone with train_flank): small
// bonuses for teammates out of sight or >= 100 units away and for each
// opponent that cannot see the agent (judged with the agent's own aim),
// hits / kills from behind the target, exploration.  CombatState is taken
// by value there, so nothing is cleared.
template <class LBVH>
__device__ __forceinline__ float flankRewardD(const DevState &S, const SceneDev &sc, const LBVH &bvh, int w, int i)
{
    const int T = S.T, N = S.N;
    const int64_t g0 = (int64_t)w * N;
    const int64_t g = g0 + i;
    const int team = i / T, off = i - team * T;
    const Vec3 pos = ldPos(S, g);
    const Quat aim_rot = ldAimRot(S, g);
    float r = 0.f;
    Vec3 vis = pos;
    vis.z += viewHeightD(S.curPose[g]);
    const float flank_dist = 100.f;
    float mates = 0.f;
    for (int k = 0; k < T - 1; k++) {
        const int j = team * T + (k < off ? k : k + 1);
        const Vec3 dir = ldPos(S, g0 + j) - pos;
        const bool seen = isAgentVisibleD(S, sc, bvh, w, vis, aim_rot, j);
        if (length2(dir) >= flank_dist * flank_dist || !seen) mates += 0.001f;
    }
    r += mates;
    float opps = 0.f;
    for (int k = 0; k < T; k++) {
        const int64_t go = g0 + (team ^ 1) * T + k;
        Vec3 op_pos = ldPos(S, go);
        op_pos.z += viewHeightD(S.curPose[go]);
        if (!isAgentVisibleD(S, sc, bvh, w, op_pos, aim_rot, i)) opps += 0.001f;
    }
    r += opps;
    const int landed = S.landedOn[g];
    if (landed != -1) {
        const float yaw_diff = fabs_(S.ayaw[g0 + landed] - S.ayaw[g]);
        if (yaw_diff > kPi) r += (S.flags[g] & kFlagSuccessfulKill) ? 1.f : 0.2f;
    }
    uint32_t nn = (uint32_t)S.newCells[g];
    S.newCells[g] = 0;
    if (nn > 0) r += float(nn) * S.rewardCoefs[9 * g + 2];
    S.reward[g] = r;
    return r;
}

// The global-resident images, once per scene upload: one block runs the
// staging loops of stageBVHSphere (whose image begins with stageBVH's) and
// stageBVHOct into the two buffers, so the bytes are those a block of the
// LDS path stages for itself.
__global__ void __launch_bounds__(kBlock) k_scene_images(SceneDev sc, SceneImages img)
{
    (void)stageBVHSphere<LBVHG, true>(img.sphere, sc);
    (void)stageBVHOct<LBVHG, true>(img.oct, sc);
}

// Copy one step of the action tape ([A][6] i32: 4 discrete + 2 aim) into the
// engine's action columns (the cudaCopyStepInputs of gpuStreamStep,
// mgr.cpp:625).
__global__ void __launch_bounds__(256) k_fill_actions(DevState S, const int32_t *src)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= S.A) return;
    const int32_t *s = src + 6 * g;
    int4 d = make_int4(s[0], s[1], s[2], s[3]);
    reinterpret_cast<int4 *>(S.discreteAction)[g] = d;
    reinterpret_cast<int2 *>(S.discreteAim)[g] = make_int2(s[4], s[5]);
}

// Synthetic combat action source (bench / tests; no reference counterpart):
// the tape row of each agent, overridden by a greedy aim-bot that reads the
// agent's current observations -- the same function as the tests'
// mpenv_testlib.combat_actions (mode 0) / seek_combat_actions (mode 1), so
// engine and oracle see identical actions while parity holds.
//   an opponent visible (first k with OPPONENT_MASKS[k] > 0): discrete aim
//   toward its relative yaw / pitch (opponent obs 24 / 25) through the
//   pvpDiscreteAimSystem turn tables (sim.cpp:2284-2370), fire iff
//   |yaw| < 0.05;  mode 1 and none visible: turn toward the zone (self obs
//   31, toCenterYaw) and run forward once within 0.5 rad of it, else stand;
//   mode 1 also reloads an empty magazine (self obs 24 == 0, not reloading).
// The bucket compares run in double against the double turn tables, as
// numpy does with its float64 tables.
__device__ __forceinline__ int32_t aimBucketD(float delta, bool yaw_table, int32_t centre)
{
    const double mag = (double)fabsf(delta);
    const double pi = 3.141592653589793;
    int32_t idx = 0;
    if (yaw_table) {
        idx += (1.0 / 256.0) * pi <= mag; idx += (1.0 / 128.0) * pi <= mag; idx += (1.0 / 64.0) * pi <= mag;
        idx += (1.0 / 32.0) * pi <= mag; idx += (1.0 / 16.0) * pi <= mag; idx += (1.0 / 8.0) * pi <= mag;
    } else {
        idx += (1.0 / 128.0) * pi <= mag; idx += (1.0 / 64.0) * pi <= mag; idx += (1.0 / 32.0) * pi <= mag;
    }
    return delta > 0.f ? centre + idx : (delta < 0.f ? centre - idx : centre);
}

__global__ void __launch_bounds__(256) k_combat_actions(DevState S, const int32_t *tape, int32_t *out, int32_t mode)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= S.A) return;
    const int32_t *t = tape + 6 * g;
    int32_t a[6] = { t[0], t[1], t[2], t[3], t[4], t[5] };
    const float *mk = S.masks + 6 * g;
    int k = -1;
    for (int j = 5; j >= 0; j--)
        if (mk[j] > 0.f) k = j;
    if (k >= 0) {
        const float *ob = S.oppObs + (g * 6 + k) * kOtherObs;
        const float yaw = ob[24], pitch = ob[25];
        a[4] = aimBucketD(yaw, true, 6);
        a[5] = aimBucketD(pitch, false, 3);
        a[2] = fabsf(yaw) < 0.05f ? 1 : 0;
    } else if (mode == 1) {
        const float zy = S.selfObs[g * kSelfObs + 31];
        a[4] = aimBucketD(zy, true, 6);
        if (fabsf(zy) < 0.5f) { a[0] = 2; a[1] = 0; } else { a[0] = 0; }
    }
    // mode 1: an empty magazine that is not already reloading is reloaded
    // (self obs 24 / 25: bullets, reload steps left)
    if (mode == 1 && S.selfObs[g * kSelfObs + 24] == 0.f && S.selfObs[g * kSelfObs + 25] == 0.f) a[2] = 2;
    if (out) {
        int32_t *o = out + 6 * g;
        for (int j = 0; j < 6; j++) o[j] = a[j];
    } else {
        reinterpret_cast<int4 *>(S.discreteAction)[g] = make_int4(a[0], a[1], a[2], a[3]);
        reinterpret_cast<int2 *>(S.discreteAim)[g] = make_int2(a[4], a[5]);
    }
}

// ============================================================ host side
const char *kernelName(int k)
{
    static const char *names[kNumTimedKernels] = { "k_move", "k_sim", "k_vis", "k_obs", "k_lidar" };
    return (k >= 0 && k < kNumTimedKernels) ? names[k] : "?";
}

size_t bvhLdsBytes(const SceneDev &sc) { return CollisionImage { sc.numNodes, sc.numVerts }.bytes(); }
size_t bvhLdsBytesSphere(const SceneDev &sc) { return SphereImage { { sc.numNodes, sc.numVerts } }.bytes(); }
size_t bvhLdsBytesOct(const SceneDev &sc) { return OctImage { sc.numLidarNodes, sc.numLidarVerts }.bytes(); }

// The step kernels' dynamic LDS under a residency: global-resident, only
// what a kernel keeps beside the image is left.
size_t simLdsBytes(const SceneDev &sc, int32_t residency)
{
    const size_t off = residency == kResidencyGlobal ? simSpawnOffset<false>(sc) : simSpawnOffset<true>(sc);
    return off + (size_t)(sc.numA + sc.numB + sc.numCommon) * sizeof(Spawn);
}

int buildSceneImages(const SceneDev &sc, const SceneImages &img, void *stream)
{
    hipLaunchKernelGGL(k_scene_images, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, sc, img);
    int rc = check(hipGetLastError());
    if (!rc) rc = check(hipStreamSynchronize((hipStream_t)stream));
    return rc;
}

int launchConstruct(const DevState &s, const SceneDev &sc, const int32_t tc[3], void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = s.A * kExploreTiles;
    int blocks = (int)std::min<int64_t>((total + 255) / 256, 65536);
    hipLaunchKernelGGL(k_init_explore, dim3(blocks), dim3(256), 0, st, s, total);
    if (check(hipGetLastError())) return -1;
    hipLaunchKernelGGL(k_construct, dim3((s.W + 63) / 64), dim3(64), 0, st, s, sc, tc[0], tc[1], tc[2]);
    return check(hipGetLastError());
}

int launchResetOnly(const DevState &s, const SceneDev &sc, void *stream)
{
    hipLaunchKernelGGL(k_reset_only, dim3((s.W + 63) / 64), dim3(64), 0, (hipStream_t)stream, s, sc);
    return check(hipGetLastError());
}

int launchSimStep(const DevState &s, const SceneDev &sc, const SceneImages &img, void *stream)
{
    const int wpb = kSimBlock / s.N;
    const int blocks = (s.W + wpb - 1) / wpb;
    return launchByResidency(img, k_sim, k_sim_g, dim3(blocks), dim3(kSimBlock), simLdsBytes(sc, img.residency),
                             stream, s, sc);
}

int computeSceneFrames(SceneTables *d_tab, void *stream)
{
    hipLaunchKernelGGL(k_scene_frames, dim3(1), dim3(64), 0, (hipStream_t)stream, d_tab);
    int rc = check(hipGetLastError());
    if (!rc) rc = check(hipStreamSynchronize((hipStream_t)stream));
    return rc;
}

int computeZoneGoalTris(const SceneDev &sc, int32_t *dev_scratch, int32_t *host_out, void *stream)
{
    hipLaunchKernelGGL(k_zone_goals, dim3(1), dim3(64), 0, (hipStream_t)stream, sc, dev_scratch);
    int rc = check(hipGetLastError());
    if (!rc) rc = check(hipMemcpyAsync(host_out, dev_scratch, sizeof(int32_t) * sc.numZones, hipMemcpyDeviceToHost,
                                       (hipStream_t)stream));
    if (!rc) rc = check(hipStreamSynchronize((hipStream_t)stream));
    return rc;
}

int launchFillActions(const DevState &s, const int32_t *src6, void *stream)
{
    hipLaunchKernelGGL(k_fill_actions, dim3((unsigned)((s.A + 255) / 256)), dim3(256), 0, (hipStream_t)stream, s,
                       src6);
    return check(hipGetLastError());
}

int launchCombatActions(const DevState &s, const int32_t *tape6, int32_t *out6, int32_t mode, void *stream)
{
    hipLaunchKernelGGL(k_combat_actions, dim3((unsigned)((s.A + 255) / 256)), dim3(256), 0, (hipStream_t)stream, s,
                       tape6, out6, mode);
    return check(hipGetLastError());
}

} // namespace mpenv
