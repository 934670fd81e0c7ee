// move.hip — k_move: the per-agent systems of the step (bots, movement, aim,
// sphere casts, fall), which read no other agent's state.
#include "casts_dev.h"
#include "nav_dev.h"

namespace mpenv {

// ====================================================== per-agent systems
// planAStarAISystem (sim.cpp:5041-5172); its NavUtils are in nav_dev.h
__device__ __forceinline__ void planAStarD(const DevState &S, const SceneDev &sc, int64_t g)
{
    if (S.policy[g] != -1) return; // consts::aStarPolicyID
    const int w = (int)(g / S.N);
    RNG rng = ldRng(S, g);
    int move_amount = rngI32(rng, 0, 2);
    int move_angle = rngI32(rng, 0, 2);
    int r_yaw = rngI32(rng, 0, 5);
    const int r_pitch = rngI32(rng, 0, 2);
    const int reload = S.magazine[2 * g] == 0 ? 1 : 0;
    int stand = rngI32(rng, 0, 2);
    stRng(S, g, rng);
    // fire if any opponent is visible (OpponentsVisibility of the last step)
    int fire = (S.visMask[g] & ((1u << S.T) - 1u)) != 0 ? 1 : 0;

    const int zi = S.curZone[w];
    const AABB z = sc.tab->zoneAABB[zi];
    Vec3 center = (z.pMin + z.pMax) / 2.f; // AABB::centroid
    const Vec3 pos = v3(S.px[g], S.py[g], 0.f);
    center = pathfindToPointD(sc, pos, center, sc.tab->zoneGoalTri[zi]);
    center.z = 0.f;
    const float yaw = S.ayaw[g];
    const Vec3 fwd = v3(-sinf_(yaw), cosf_(yaw), 0.f);
    const Vec3 tgt = normalize(center - pos);
    move_amount = dot(fwd, tgt) > 0.6f ? 1 : 0;
    r_yaw = cross(fwd, tgt).z < 0.0f ? 0 + move_amount : 4 - move_amount;
    move_amount *= 2;
    move_angle = 0;
    stand = 0;

    // wall avoidance from last step's forward lidar depths
    float coll_ang = 0.f, coll_norm = 0.f;
    const float *lid = &S.fwdLidar[g * kFwdRays * 4];
    for (int y = 0; y < 2; y++) {
        for (int x = 0; x < 32; x++) {
            if (lid[(y * 32 + x) * 4] < 16.0f) {
                coll_norm++;
                coll_ang += x;
            }
        }
    }
    if (coll_norm > 0.f) {
        coll_ang /= coll_norm;
        move_amount = 1;
        switch ((int)(coll_ang / 32.f * 8.0f)) {
        case 0: move_angle = 2; break;
        case 1:
        case 2: move_angle = 3; break;
        case 3:
        case 4: move_angle = 4; move_amount = 2; break;
        case 5:
        case 6: move_angle = 5; break;
        case 7: move_angle = 6; break;
        }
    }
    if (reload) fire = 0;
    if (fire) r_yaw = 2;
    int32_t *out = &S.botAction[7 * g];
    out[0] = move_amount;
    out[1] = move_angle;
    out[2] = r_yaw;
    out[3] = r_pitch;
    out[4] = fire;
    out[5] = reload;
    out[6] = stand;
}

// sim.cpp:2057-2091 applyBotActionsSystem
__device__ __forceinline__ void applyBotActionsD(const DevState &S, int64_t g)
{
    if (S.policy[g] != -1) return;
    const int32_t *hb = &S.botAction[7 * g];
    S.discreteAction[4 * g + 0] = hb[0];
    S.discreteAction[4 * g + 1] = hb[1];
    S.discreteAction[4 * g + 2] = hb[4];
    S.discreteAction[4 * g + 3] = hb[6];
    const float turn_delta = 10.f / (float)(5 / 2);
    S.aimAction[2 * g] = turn_delta * (float)(hb[2] - 5 / 2);
    S.aimAction[2 * g + 1] = turn_delta * (float)(hb[3] - 5 / 2);
}

// sim.cpp:2093-2199 pvpMovementSystem
__device__ __forceinline__ void pvpMovementD(const DevState &S, int64_t g)
{
    if (S.alive[g] == 0.f) return;
    const int32_t a_amount = S.discreteAction[4 * g + 0];
    const int32_t a_angle = S.discreteAction[4 * g + 1];
    const int32_t a_stand = S.discreteAction[4 * g + 3];
    Vec3 vel = ldVel(S, g);
    {
        float v_len = length(vel);
        if (v_len > 0.f) {
            Vec3 norm_v = vel / v_len;
            v_len -= c::kDeaccelerateRate * c::kDeltaT;
            v_len = fmaxD(0.f, v_len);
            vel = norm_v * v_len;
        }
    }
    int cur = S.curPose[g], tgt = S.tgtPose[g], tr = S.transRem[g];
    if (tr > 0) {
        tr -= 1;
        if (tr == 0) cur = tgt;
    }
    if (a_stand != tgt) {
        tgt = a_stand;
        int dst = tgt - cur;
        dst = dst < 0 ? -dst : dst;
        tr = dst * (c::kPoseTransitionSpeed / 2);
    }
    S.curPose[g] = cur; S.tgtPose[g] = tgt; S.transRem[g] = tr;

    float accel_max = 3000;
    if (cur == kCrouch) accel_max = 100;
    else if (cur == kProne) accel_max = 50;
    float move_amount = (float)a_amount * (accel_max / (float)(c::kNumMoveAmountBuckets - 1));
    const float per_bucket = 2.f * kPi / float(c::kNumMoveAngleBuckets);
    float move_angle = float(a_angle) * per_bucket;
    float f_x = move_amount * sinf_(move_angle);
    float f_y = move_amount * cosf_(move_angle);
    vel = vel + rotateVec(ldRot(S, g), v3(f_x, f_y, 0)) * c::kDeltaT;
    if (move_amount != 0) S.respawnSteps[g] = 0;
    float v_len = length(vel);
    if (v_len == 0.f) {
        stVel(S, g, vel);
        return;
    }
    float max_vel = S.maxVel[g];
    {
        const float max_change = 510.f;
        float tgt_v;
        if (cur == kStand) tgt_v = a_amount == 2 ? c::kMaxRunVelocity : c::kMaxWalkVelocity;
        else if (cur == kCrouch) tgt_v = c::kMaxCrouchVelocity;
        else tgt_v = c::kMaxProneVelocity;
        float diff = tgt_v - max_vel;
        float adj = fmaxD(fminD(diff, max_change), -max_change);
        max_vel += adj;
    }
    S.maxVel[g] = max_vel;
    Vec3 v_norm = vel / v_len;
    v_len = fminD(v_len, max_vel);
    stVel(S, g, v_norm * v_len);
}

// sim.cpp:2266-2370 continuous then discrete aim
__device__ __forceinline__ void pvpAimD(const DevState &S, int64_t g)
{
    if (S.alive[g] == 0.f) return;
    float yaw = S.ayaw[g], pitch = S.apitch[g];
    yaw += S.aimAction[2 * g] * c::kDeltaT;
    pitch += S.aimAction[2 * g + 1] * c::kDeltaT;
    AimD a = computeAimD(yaw, pitch);
    yaw = a.yaw; pitch = a.pitch;
    // pvpContinuousAimSystem writes Rotation too; it is overwritten below.
    const float yaw_turn[7] = { 0, 0.00390625f * kPi, 0.0078125f * kPi, 0.015625f * kPi,
                                0.03125f * kPi, 0.0625f * kPi, 0.125f * kPi };
    const float pitch_turn[4] = { 0, 0.0078125f * kPi, 0.015625f * kPi, 0.03125f * kPi };
    int yb = S.discreteAim[2 * g] - c::kDiscreteAimYawBuckets / 2;
    int yba = yb < 0 ? -yb : yb;
    if (yb < 0) yaw -= yaw_turn[yba];
    else yaw += yaw_turn[yba];
    int pb = S.discreteAim[2 * g + 1] - c::kDiscreteAimPitchBuckets / 2;
    int pba = pb < 0 ? -pb : pb;
    if (pb < 0) pitch -= pitch_turn[pba];
    else pitch += pitch_turn[pba];
    a = computeAimD(yaw, pitch);
    stAim(S, g, a);
    stRot(S, g, qnormalize(angleAxis(a.yaw, kUp)));
}

// sim.cpp:889-1039 applyVelocitySystem + updateMoveStateSystem.  Split at
// the stuck fallback so the wave can share its casts (stuckCastsD): part 1
// up to the ground check, the fallback's casts, part 2 to the end.
template <class LBVH>
__device__ __forceinline__ void applyVelocityD(const DevState &S, const SceneDev &sc, const LBVH &bvh, int64_t g)
{
    const Vec3 x = ldPos(S, g);
    Vec3 v = ldVel(S, g);
    v.z = 0;
    Vec3 new_pos = x;
    Vec3 new_vel = v3(0.f, 0.f, 0.f);
    const int pose = S.curPose[g];
    float v_len = length(v);
    const float buffer = 0.05f * c::kAgentRadius;
    const float r = c::kAgentRadius;
    float top = c::kStandHeight - r;
    float low_check = c::kProneHeight;
    if (pose == kCrouch) {
        top = c::kCrouchHeight - r;
    } else if (pose == kProne) {
        top = low_check;
        low_check = c::kProneHeight - r + buffer;
    }
    Vec3 v_norm = v3(0.f, 0.f, 0.f);
    Vec3 hit_pos = x, ground_check = x;
    float ground_dist = 0.f;
    bool cont = false, stuck_path = false;
    do {
        if (v_len == 0.f) break;
        v_norm = v / v_len;
        float move_dist = v_len * c::kDeltaT;

        Vec3 ray_o = x;
        ray_o.z += top;
        Vec3 normal = v3(0.f, 0.f, 0.f);
        {
            // the ground below, wherever it is (a bounded first try gains
            // nothing here: the downward cast prunes at the floor anyway)
            SphereHit h = bvhSphereCastD(bvh, ray_o, -kUp, r);
            if (h.t < kFltMax) normal = h.n;
        }
        if (normal.z > 0.0f && (double)normal.z < 0.7 && dot(normal, v_norm) < 0.0f) break;

        // The forward casts only matter nearer than move_dist + buffer: a
        // farther hit leaves hit_pos at move_dist, takes no slide and the
        // normal / high_hit it sets are read only by the slide (bound with a
        // margin of kCastSlack so no value near a decision is ever cut).
        const float fwd_b = (move_dist + buffer) + kCastSlack;
        ray_o = x + v_norm * buffer * 0.5f;
        ray_o.z += low_check;
        // the low cast and (standing / crouching) the high cast from
        // (ray_o.xy, x.z + top), traversed together
        SphereHit hl, hh;
        hh.t = kFltMax;
        castNear2D(bvh, sc, ray_o, x.z + top, v_norm, fwd_b, pose != kProne, hl, hh);
        float low_dist = hl.t;
        if (hl.t < kFltMax) normal = hl.n;
        float high_dist = low_dist;
        bool high_hit = false;
        if (pose != kProne) {
            high_dist = hh.t;
            if (high_dist < low_dist) {
                low_dist = high_dist;
                normal = hh.n;
                high_hit = true;
            }
        }
        bool stuck = low_dist == 0.0f || high_dist == 0.0f;
        low_dist = fmaxD(0.0f, low_dist - buffer);
        high_dist = fmaxD(0.0f, high_dist - buffer);
        hit_pos = x + v_norm * fminD(low_dist, move_dist);

        if (move_dist > low_dist) {
            Vec3 slide_dir = normalize(cross(kUp, normal));
            if (dot(slide_dir, v_norm) < 0) slide_dir = -slide_dir;
            ray_o = x + v_norm * low_dist;
            ray_o.z += high_hit ? top : low_check;
            float max_move = move_dist - low_dist;
            // only min(slide - buffer, max_move) is used
            float slide = castNearD(bvh, sc, ray_o, slide_dir, (max_move + buffer) + kCastSlack).t;
            slide = fmaxD(0.0f, slide - buffer);
            slide = fminD(slide, max_move);
            if (slide > 0.0f) hit_pos = hit_pos + slide_dir * slide;
        }

        ground_check = hit_pos;
        ground_check.z += top;
        // min(ground_dist, top) is used, and whether there is ground at all
        ground_dist = castFirstNearD(bvh, sc, ground_check, -kUp, 2.f * top + 10.f);
        if (ground_dist == kFltMax) break;
        stuck_path = (ground_dist <= 0.0f || stuck);
        cont = true;
    } while (false);

    float hd4[4] = { 0.f, 0.f, 0.f, 0.f };
    stuckCastsD(bvh, stuck_path, x, v_norm, low_check, hd4);

    while (cont) {
        if (stuck_path) {
            float furthest = 0.0f;
            int best_dir = -1;
            for (int dir = 0; dir < 4; dir++) {
                if (hd4[dir] > furthest) {
                    furthest = hd4[dir];
                    best_dir = dir;
                }
            }
            if (best_dir != -1) {
                Vec3 dv = rotate2DD(v_norm, (float)best_dir * 3.14159f * 0.5f);
                hit_pos = x + dv * (fminD(furthest - r * 2.0f, -buffer));
                ground_check = hit_pos;
                ground_check.z += top;
                ground_dist = bvhSphereCastD(bvh, ground_check, -kUp, r).t;
                if (ground_dist == kFltMax) break;
            }
        }

        float fall_dist = fminD(ground_dist, top) + r;
        Vec3 np = ground_check;
        np.z -= fall_dist;
        Vec3 to_new = np - x;
        float to_new_dist = length(to_new);
        if (to_new_dist == 0.f) break;
        new_pos = np;
        new_vel = to_new / c::kDeltaT;
        break;
    }
    // updateMoveStateSystem (sim.cpp:1030-1039)
    stPos(S, g, new_pos);
    stVel(S, g, new_vel);
}

// sim.cpp:1041-1104 fallSystem + updateMoveStatePostFallSystem
template <class LBVH>
__device__ __forceinline__ void fallD(const DevState &S, const SceneDev &sc, const LBVH &bvh, int64_t g)
{
    if (S.alive[g] == 0.f) return;
    const float fall_rate = 386.08858267717f;
    const float cast_offset = c::kAgentRadius;
    Vec3 pos = ldPos(S, g);
    Vec3 ray_o = pos;
    ray_o.z += c::kAgentRadius + cast_offset;
    // min(ground - cast_offset, fall_rate * dt) is used, and whether there
    // is ground at all
    float ground = castFirstNearD(bvh, sc, ray_o, -kUp, 2.f * (cast_offset + fall_rate * c::kDeltaT) + 10.f);
    if (ground == kFltMax || ground < cast_offset) return;
    float fall = fminD(ground - cast_offset, fall_rate * c::kDeltaT);
    pos.z -= fall;
    S.pz[g] = pos.z;
}

// Step graph part 1 (sim.cpp:5299-5320 up to updateMoveStatePostFall): the
// per-agent systems, which read no other agent's state.  Lane = agent, no
// barriers, so sphere-cast latency overlaps across the whole grid.
// apw: agents per wave (64, or fewer on small batches: a wave runs the
// longest of its lanes' sphere-cast chains, so when the batch leaves SIMDs
// idle, fewer agents per wave shorten every wave; launchMove picks it).
template <class LBVH>
__device__ __forceinline__ void moveBody(const DevState &S, const SceneDev &sc, int apw, char *img)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    LBVH bvh = stageBVHSphere<LBVH>(LBVH::kStaged ? smem : img, sc);
    bvh.stats = S.stats;
    [&]() {
        const int lane = threadIdx.x & 63;
        if (lane >= apw) return;
        const int64_t wave = ((int64_t)xcdBlockId() * blockDim.x + threadIdx.x) >> 6;
        const int64_t g = wave * apw + lane;
        if (g >= S.A) return;
        if (S.stats) statAdd(S.stats + kStatAliveAgents, S.alive[g] != 0.f ? 1u : 0u);
        planAStarD(S, sc, g);
        if (sc.replayOn) return; // pvpReplayLogic replaces the gameplay systems (sim.cpp:5587-5605)
        applyBotActionsD(S, g);
        pvpMovementD(S, g);
        pvpAimD(S, g);
        applyVelocityD(S, sc, bvh, g);
        fallD(S, sc, bvh, g);
    }();
}

// Each kernel that walks a BVH is its body instantiated over the LDS view and
// (`_g`, with the images as one more argument) over the global one; the host
// launcher picks by SceneImages::residency.
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(3))) k_move(DevState S, SceneDev sc, int apw)
{
    moveBody<LBVHL>(S, sc, apw, nullptr);
}

__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(3))) k_move_g(DevState S, SceneDev sc, int apw, SceneImages img)
{
    moveBody<LBVHG>(S, sc, apw, img.sphere);
}

// ============================================================ host side
static_assert(c::kAgentRadius == kSphereR, "k_move sphere casts use the agent radius (stageBVHSphere)");

size_t moveLdsBytes(const SceneDev &sc, int32_t residency)
{
    return residency == kResidencyGlobal ? 0 : bvhLdsBytesSphere(sc);
}

int launchMove(const DevState &s, const SceneDev &sc, const SceneImages &img, void *stream)
{
    // Small batches (< 64 full blocks): one-wave blocks, so the few waves spread over CUs
    // instead of sharing a CU's SIMDs (k_move is latency-bound: 5-7
    // dependent sphere casts per lane).  Big batches keep 256-thread blocks
    // (the 24 KB LDS image per block would otherwise cap occupancy).
    // Agents per wave: 64 once the batch fills ~1.5 waves per SIMD (1,536
    // waves on 256 CUs), else the power of two (>= 8) that gets closest.
    int apw = 64;
    while (apw > 8 && (s.A + apw - 1) / apw < 1536) apw >>= 1;
    const int64_t waves = (s.A + apw - 1) / apw;
    const int bs = waves < 64 * 4 ? 64 : kBlock;
    const int64_t threads = waves * 64;
    return launchByResidency(img, k_move, k_move_g, dim3((unsigned)((threads + bs - 1) / bs)), dim3(bs),
                             moveLdsBytes(sc, img.residency), stream, s, sc, apw);
}

} // namespace mpenv
