// lidar.hip — k_lidar: 80 lidar rays per agent.
#include "sim_dev.h"

namespace mpenv {

// pvpLidarSystem (sim.cpp:3324-3506).  Lane = ray.  Rays are dealt to
// waves in units of 4 agents = 5 wave tasks: tasks 0-3 carry one agent's 64
// forward rays each (32 angles x 2 heights, one origin and a narrow fan, so
// the wave's lanes walk similar BVH paths), task 4 the 4 agents' 16 rear rays.
// Against 64 consecutive rays of the flat [agent][80] order (which straddle
// two agents in 4 of 5 waves) this cuts the wave-lockstep node iterations by
// ~12% and triangle tests by ~19% (tools/trav_stats.cpp on recorded rays);
// every lane's arithmetic is unchanged.  A block owns `iters` x 16
// consecutive tasks and its 16 waves draw them one at a time from a counter
// in LDS, so a wave that drew short tasks takes more of them and the block's
// LDS image is not held for the wave with the longest fixed share (DESIGN.md
// §4, "k_lidar's task scheduling").  `iters` is up to kLidarItersAuto (amortises the BVH staging) on big
// batches, fewer on small ones so the grid still spreads over the CUs (at 64
// worlds 1v1 a fixed 8 put the whole lidar on 5 CUs): lidarItersFor.
constexpr int kLidarIters = 12;    // compiled maximum of tasks per wave (mpenv_set_lidar_iters)
constexpr int kLidarItersAuto = 6; // what launchLidar's caller gets on big batches: round 5, one world group: 4: 0.665, 5: 0.642, 6: 0.643 ms steady (profiles/r05m_lab_lidar_iters.jsonl; round 2: 1: 0.98, 2: 0.91, 4: 0.89, 8: 0.92 ms)
// 1024-thread blocks: the 8 octant node images + the three rotated vertex
// copies (31 + 36 KB on simple_map) are staged once per 16 waves, so 2
// blocks per CU (8 waves per SIMD) fit the 160 KB of LDS: 67 KB of image
// plus 9,168 B of static LDS (the agent stage, sized for kLidarIters = 12
// tasks per wave: 8,832 B; 5,376 B when the maximum was 6) is ~76 KB per
// block, 152 KB for two, 8 KB of headroom.
constexpr int kLidarBlock = 1024;
constexpr int kLidarWaves = kLidarBlock / 64;
constexpr int kLidarStageMax = 184, kLidarStageCols = 12; // k_lidar's per-block agent stage
static_assert(4 * ((kLidarIters * kLidarWaves) / 5 + 2) + 2 * (2 * kMaxTeamSize - 1) <= kLidarStageMax,
              "k_lidar agent stage");

__device__ __host__ __forceinline__ int64_t lidarTasks(int64_t A) { return ((A + 3) / 4) * 5; }

// 8 waves per SIMD (64 VGPRs, a few bytes of spill outside the traversal
// loop): latency-bound LDS traversal gains more from occupancy (-7%).
#define MP_LIDAR_ATTR __attribute__((amdgpu_waves_per_eu(8)))

// Maximum over the lane's DPP row (16 lanes) of non-negative float bit
// patterns compared as signed ints (the float order; -0 sorts lowest): the
// exact float maximum of the row's hit distances, without LDS round trips.
__device__ __forceinline__ int rowMaxBits16(int v)
{
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false));  // quad_perm [1, 0, 3, 2]
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false));  // quad_perm [2, 3, 0, 1]
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x124, 0xF, 0xF, false)); // row_ror:4
    return max(v, __builtin_amdgcn_update_dpp(0, v, 0x128, 0xF, 0xF, false)); // row_ror:8
}

template <class LBVH>
__device__ __forceinline__ void lidarBody(const DevState &S, const SceneDev &sc, int iters, char *img)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // Ray-fan directions (sim.cpp:3324-3506): theta depends only on the ray
    // slot, so the 32 forward + 8 rear (-cos, sin) pairs are computed once
    // per workgroup with the same sinf_/cosf_ and read from LDS.
    __shared__ float2 fan[32 + 8];
    if (threadIdx.x < 40) {
        const bool fwd = threadIdx.x < 32;
        const int x = fwd ? threadIdx.x : threadIdx.x - 32;
        const int width = fwd ? 32 : 8;
        const float range = fwd ? 0.75f * kPi : -kPi;
        const float offset = fwd ? 0.5f * (1.f - 0.75f) * kPi : 0.f;
        const float theta = range * (float(x) / float(width - 1)) + offset;
        fan[threadIdx.x] = make_float2(-cosf_(theta), sinf_(theta));
    }
    const uint32_t N = (uint32_t)S.N, T = (uint32_t)S.T;
    const uint32_t A = (uint32_t)S.A;
    const uint32_t ntasks = (uint32_t)lidarTasks(S.A);
    // The agents this block's tasks read -- the rays' origins and frames and
    // every capsule of their worlds -- staged in LDS with the BVH: whole
    // worlds around the block's task range (at kLidarIters = 12: <= 40 units
    // of 4 agents plus a partial world at each end: <= 182 agents, N <= 12;
    // the automatic 6: <= 21 units, <= 106 agents), so no task waits on HBM
    // for them.
    __shared__ float agentStage[kLidarStageCols][kLidarStageMax];
    const uint32_t t0 = xcdBlockId() * (uint32_t)iters * kLidarWaves;
    const uint32_t t1 = min(ntasks, t0 + (uint32_t)iters * kLidarWaves);
    uint32_t s0 = 0, ns = 0;
    if (t0 < t1) {
        const uint32_t a_lo = (t0 / 5u) * 4u, a_hi = min(A, ((t1 - 1u) / 5u) * 4u + 4u);
        s0 = (a_lo / N) * N;
        ns = ((a_hi - 1u) / N + 1u) * N - s0;
        for (uint32_t k = threadIdx.x; k < ns; k += blockDim.x) {
            const uint32_t g = s0 + k;
            agentStage[0][k] = S.px[g];
            agentStage[1][k] = S.py[g];
            agentStage[2][k] = S.pz[g];
            agentStage[3][k] = S.aw[g];
            agentStage[4][k] = S.ax[g];
            agentStage[5][k] = S.ay[g];
            agentStage[6][k] = S.az[g];
            agentStage[7][k] = S.rw[g];
            agentStage[8][k] = S.rx[g];
            agentStage[9][k] = S.ry[g];
            agentStage[10][k] = S.rz[g];
            agentStage[11][k] = viewHeightD(S.curPose[g]);
        }
    }
    // gpuStreamStep's caller buffers (engine.h OutTab), read once per block
    // into wave-uniform values (off: all null), held in scalar registers
    // across the traversals
    float4 *oFwd = nullptr, *oRear = nullptr, *oMap0 = nullptr, *oMap1 = nullptr;
    if (S.outTab && S.outTab->on) {
        auto uniform = [](const float *p) {
            const uint64_t v = reinterpret_cast<uint64_t>(p);
            const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
            const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
            return reinterpret_cast<float4 *>(((uint64_t)hi << 32) | lo);
        };
        oFwd = uniform(S.outTab->fwdLidar);
        oRear = uniform(S.outTab->rearLidar);
        oMap0 = uniform(S.outTab->agentMap0);
        oMap1 = uniform(S.outTab->agentMap1);
    }
    // The block's tasks are dealt from this counter: wave v starts with task
    // v of the block; a wave that is free draws the next one (one LDS atomic
    // by lane 0, broadcast), and leaves when the range is used up.  No wave
    // ever waits for another.  With one task per wave nothing is drawn.
    __shared__ uint32_t nextTask;
    if (threadIdx.x == 0) nextTask = kLidarWaves;
    const LBVH bvh = stageBVHOct<LBVH>(LBVH::kStaged ? smem : img, sc); // ends with __syncthreads
    auto draw = [&]() {
        if (iters == 1) return (uint32_t)kLidarWaves;
        // the lane id read here (volatile, as in the loop body): hoisted out
        // of the loop it lived across the traversal and was spilled
        uint32_t ln, drawn = 0u;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
        if (ln == 0u) drawn = atomicAdd(&nextTask, 1u);
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)drawn);
    };
    for (uint32_t k = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); t0 + k < t1; k = draw()) {
        const uint32_t task = t0 + k; // wave-uniform
        const uint32_t unit = task / 5u, sub = task - unit * 5u;
        const bool fwd = sub < 4u;
        // The ray of lane `ln`: a tail unit's lanes past A trace a copy of
        // the last agent's rays and store nothing.
        auto rayIndex = [&](uint32_t ln, uint32_t &g, bool &valid, uint32_t &kk) {
            const uint32_t g_raw = unit * 4u + (fwd ? sub : (ln >> 4));
            valid = g_raw < A;
            g = min(g_raw, A - 1u); // (a min with a scalar: a select kept A - 1 in a VGPR across the loop)
            kk = fwd ? ln : (ln & 15u); // ray slot within the forward / rear fan
        };
        auto makeRay = [&](uint32_t ln, uint32_t &g, bool &valid, uint32_t &kk, Vec3 &ray_o, Vec3 &dir) {
            rayIndex(ln, g, valid, kk);
            const uint32_t h = fwd ? (kk >> 5) : (kk >> 3), x = fwd ? (kk & 31u) : (kk & 7u);
            const uint32_t k = g - s0, qc = fwd ? 3u : 7u;
            const Quat q = quat(agentStage[qc][k], agentStage[qc + 1u][k], agentStage[qc + 2u][k],
                                agentStage[qc + 3u][k]);
            const Vec3 dir_fwd = rotateVec(q, kFwd);
            const Vec3 dir_right = rotateVec(q, kRight);
            const float top = agentStage[11][k] + c::kAgentRadius;
            ray_o = v3(agentStage[0][k], agentStage[1][k], agentStage[2][k]);
            ray_o.z += c::kAgentRadius + (top - 2.f * c::kAgentRadius) * (float(h) / float(2 - 1));
            const float2 cs = fan[fwd ? x : 32 + x];
            dir = normalize(cs.x * dir_right + cs.y * dir_fwd);
        };
        // Lane id read inside the loop (volatile: not hoisted), so the
        // lane-derived offsets are formed per task instead of living as
        // loop invariants across the traversal, which at 64 VGPRs the
        // compiler would spill to scratch.
        uint32_t lane;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
        uint32_t g, kk;
        bool valid;
        Vec3 ray_o, dir;
        // The BVH first (one traversal for both fan kinds), then the world's
        // capsules.  World / agent indices are formed after the traversal,
        // from an opaque copy of g (nothing but the ray lives across it).
        float tb;
        bool bhit;
        {
            makeRay(lane, g, valid, kk, ray_o, dir);
            // the ray's octant image: same nodes and leaves, near-first slot
            // order (scene.h octantNodeImages)
            LBVH ob = bvh;
            ob.nodes = reinterpret_cast<const MP_LDS BVHNode *>(reinterpret_cast<const MP_LDS uint4 *>(bvh.nodes) +
                                                                 rayOctant(dir) * sc.numLidarNodes * kOctNodeQ);
            bhit = bvhTraceRayT<false, kOctNodeQ, true, true>(ob, ray_o, dir, tb, kFltMax, 0.f);
        }
        // The lane id again (volatile) and the ray's indices from it: integer
        // work only, so they need not live across the traversal (at 64 VGPRs
        // they were spilled to scratch).  Shuffles below address lanes from
        // this id too (ds_bpermute), not from a lane id kept for the kernel.
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
        rayIndex(lane, g, valid, kk);
        auto shflLane = [](float v, uint32_t src) {
            return __int_as_float(__builtin_amdgcn_ds_bpermute((int)(src << 2), __float_as_int(v)));
        };
        const uint32_t w = __umulhi(g, S.nMagic); // g / N (engine.h)
        const uint32_t i = g - w * N;
        const int64_t g0 = (int64_t)w * N;
        WorldHit hw;
        if (fwd) {
            // Forward fan (one agent, one xy origin per wave): the BVH first,
            // then only the capsules some ray of the wave could hit before
            // its BVH hit.  Any point of capsule j lies within r of its
            // vertical axis, so a ray entering it at t has t >= d_xy - r
            // (d_xy = xy distance from the origin to the axis); a capsule
            // with d_xy - 1.01 r - 1 > max over the wave's rays of the BVH
            // hit t can enter no ray's `t < min_hit_t` (utils.cpp:57-69) and
            // is dropped for the whole wave (the margin dwarfs the rounding
            // of t ~ 1e-3 at these distances).  Lane j < N loads capsule j
            // once; the per-ray loop reads the survivors' bases from those
            // lanes (readlane) in ascending j, so ties resolve as before.
            float min_t = bhit ? tb : kFltMax;
            const int rm = rowMaxBits16(__float_as_int(min_t));
            const float mx = __int_as_float(max(max(__builtin_amdgcn_readlane(rm, 0), __builtin_amdgcn_readlane(rm, 16)),
                                                max(__builtin_amdgcn_readlane(rm, 32), __builtin_amdgcn_readlane(rm, 48))));
            float cx = 0.f, cy = 0.f, cz = 0.f;
            bool keep = false;
            if (lane < N) {
                const uint32_t k = (uint32_t)(g0 - s0) + lane;
                cx = agentStage[0][k]; cy = agentStage[1][k]; cz = agentStage[2][k];
                const float dx = cx - ray_o.x, dy = cy - ray_o.y;
                keep = lane != i && !(sqrtf(dx * dx + dy * dy) - c::kAgentRadius * 1.01f - 1.f > mx);
            }
            uint64_t cm = __ballot(keep);
            bool hit = bhit;
            int ent = -1;
            const float dxy2 = dir.x * dir.x + dir.y * dir.y;
            const float cull_r2 = (kCapsuleRadius * 1.01f) * (kCapsuleRadius * 1.01f);
            while (cm) {
                const int j = __builtin_ctzll(cm);
                cm &= cm - 1;
                Vec3 co = v3(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(cx), j)),
                             __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cy), j)),
                             __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cz), j)));
                co.z += kCapsuleRadius;
                const Vec3 tr = ray_o - co;
                // the per-ray conservative culls of capsulesD
                const float cr = tr.x * dir.y - tr.y * dir.x;
                if (cr * cr > cull_r2 * dxy2) continue;
                const float along = -(tr.x * dir.x + tr.y * dir.y + tr.z * dir.z);
                const float ahead = along + fmaxD(0.f, kCapsuleSegment * dir.z) + kCapsuleRadius * 1.01f;
                if (ahead < 0.f) continue;
                if (along + fminD(0.f, kCapsuleSegment * dir.z) - kCapsuleRadius * 1.01f > min_t) continue;
                const float t = intersectRayZOriginCapsule(tr, dir, kCapsuleRadius, kCapsuleSegment);
                if (t != 0 && t < min_t) {
                    min_t = t;
                    hit = true;
                    ent = j;
                }
            }
            hw.hit = hit;
            hw.t = min_t;
            hw.entity = ent;
        } else {
            // Rear fans: the same cull per 16-lane group (one agent, one xy
            // origin per group; N <= 12 capsules).  Lane q*16 + j < q*16 + N
            // loads capsule j of group q's world; the wave walks the union
            // of the groups' surviving j in ascending order and each lane
            // takes its group's copy (ds_bpermute) and tests only the j its
            // group kept -- per ray the same capsules in the same order as
            // capsulesD minus those no ray of the group can reach.
            float min_t = bhit ? tb : kFltMax;
            const float mx = __int_as_float(rowMaxBits16(__float_as_int(min_t)));
            const uint32_t gb = lane & 48u, jl = lane & 15u;
            float cx = 0.f, cy = 0.f, cz = 0.f;
            bool keep = false;
            if (jl < N) {
                const uint32_t k = (uint32_t)(g0 - s0) + jl;
                cx = agentStage[0][k]; cy = agentStage[1][k]; cz = agentStage[2][k];
                const float dx = cx - ray_o.x, dy = cy - ray_o.y;
                keep = jl != i && !(sqrtf(dx * dx + dy * dy) - c::kAgentRadius * 1.01f - 1.f > mx);
            }
            const uint64_t cm = __ballot(keep);
            uint32_t um = (uint32_t)((cm | (cm >> 16) | (cm >> 32) | (cm >> 48)) & 0xffffu);
            const uint32_t mine = (uint32_t)(cm >> gb) & 0xffffu;
            // the four agents in one world (always for 6v6: 4 divides N):
            // every group holds the same capsules, read from group 0's lanes
            const bool oneWorld = __ballot(w != (uint32_t)__builtin_amdgcn_readfirstlane((int)w)) == 0ull;
            bool hit = bhit;
            int ent = -1;
            const float dxy2 = dir.x * dir.x + dir.y * dir.y;
            const float cull_r2 = (kCapsuleRadius * 1.01f) * (kCapsuleRadius * 1.01f);
            while (um) {
                const int j = __builtin_ctz(um);
                um &= um - 1u;
                Vec3 co;
                if (oneWorld) {
                    co = v3(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(cx), j)),
                            __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cy), j)),
                            __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cz), j)));
                } else {
                    const uint32_t src = gb + (uint32_t)j;
                    co = v3(shflLane(cx, src), shflLane(cy, src), shflLane(cz, src));
                }
                if (!((mine >> j) & 1u)) continue;
                co.z += kCapsuleRadius;
                const Vec3 tr = ray_o - co;
                const float cr = tr.x * dir.y - tr.y * dir.x;
                if (cr * cr > cull_r2 * dxy2) continue;
                const float along = -(tr.x * dir.x + tr.y * dir.y + tr.z * dir.z);
                const float ahead = along + fmaxD(0.f, kCapsuleSegment * dir.z) + kCapsuleRadius * 1.01f;
                if (ahead < 0.f) continue;
                if (along + fminD(0.f, kCapsuleSegment * dir.z) - kCapsuleRadius * 1.01f > min_t) continue;
                const float t = intersectRayZOriginCapsule(tr, dir, kCapsuleRadius, kCapsuleSegment);
                if (t != 0 && t < min_t) {
                    min_t = t;
                    hit = true;
                    ent = j;
                }
            }
            hw.hit = hit;
            hw.t = min_t;
            hw.entity = ent;
        }
        if (!valid) continue;
        const bool second = i >= T; // team of the casting agent
        float4 out;
        if (hw.hit) {
            const bool wall = hw.entity == -1;
            const bool tm = !wall && ((uint32_t)hw.entity >= T) == second;
            out = make_float4(fminD(hw.t, sc.maxDist), wall ? 1.f : 0.f, tm ? 1.f : 0.f, (!wall && !tm) ? 1.f : 0.f);
        } else {
            out = make_float4(-1.f, 0.f, 0.f, 0.f);
        }
        // Addresses formed after the traversal (nothing but the ray lives
        // across it, so 64 VGPRs hold the loop without scratch spills).
        float4 *dst = fwd ? reinterpret_cast<float4 *>(S.fwdLidar) + (int64_t)g * kFwdRays + kk
                          : reinterpret_cast<float4 *>(S.rearLidar) + (int64_t)g * kRearRays + kk;
        const int64_t slot = ((int64_t)w * 2 + (second ? 1 : 0)) * kMaxTeamSize + (second ? i - T : i);
        float4 *tdst = fwd ? reinterpret_cast<float4 *>(S.ftFwdLidar) + slot * kFwdRays + kk
                           : reinterpret_cast<float4 *>(S.ftRearLidar) + slot * kRearRays + kk;
        // fullTeamObservationsSystem copies the lidar before this system
        // overwrites it (sim.cpp:5283-5310): the previous value moves into
        // the team interface's slot.  (Moving this copy into a block
        // prologue, so that the loop loads nothing, measured slower:
        // DESIGN.md §4, "k_lidar's task scheduling".)
        *tdst = *dst;
        *dst = out;
        // gpuStreamStep: the caller's lidar buffer too (the engine's copy is
        // state: the bots and the next full-team copy read it), and the
        // agent's two agent maps zero-filled by its forward wave (4 KB each:
        // 4 store instructions of 64 x 16 B per map, no loads; the stores
        // drain while the wave's next traversal runs)
        if (oFwd) {
            const int64_t gb = S.outBase + (int64_t)g;
            float4 *cdst = fwd ? oFwd + gb * kFwdRays + kk : oRear + gb * kRearRays + kk;
            *cdst = out;
            if (fwd) {
                const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
                float4 *m0 = oMap0 + gb * 256 + kk;
                float4 *m1 = oMap1 + gb * 256 + kk;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    m0[64 * q] = z;
                    m1[64 * q] = z;
                }
            }
        }
    }
}

__global__ void __launch_bounds__(kLidarBlock) MP_LIDAR_ATTR k_lidar(DevState S, SceneDev sc, int iters)
{
    lidarBody<LBVHL>(S, sc, iters, nullptr);
}

__global__ void __launch_bounds__(kLidarBlock) MP_LIDAR_ATTR k_lidar_g(DevState S, SceneDev sc, int iters, SceneImages img)
{
    lidarBody<LBVHG>(S, sc, iters, img.oct);
}

// ============================================================ host side
size_t lidarLdsBytes(const SceneDev &sc, int32_t residency)
{
    return residency == kResidencyGlobal ? 0 : bvhLdsBytesOct(sc);
}

int lidarItersMax() { return kLidarIters; }

// k_lidar's automatic tasks per wave for a batch of A agents: ~1024 blocks
// before the value grows past 1, so the grid still spreads over the CUs, and
// kLidarItersAuto at most (C3 with the waves drawing their tasks: 6: 0.579 ms,
// 10, the value with the fewest dispatch rounds on 256 CUs: 0.596 ms, DESIGN.md
// §4; larger values are for mpenv_set_lidar_iters).
int lidarItersFor(int64_t A)
{
    return (int)std::max<int64_t>(1, std::min<int64_t>(kLidarItersAuto, lidarTasks(A) / (kLidarWaves * 1024)));
}

int launchLidar(const DevState &s, const SceneDev &sc, const SceneImages &img, int iters, void *stream)
{
    if (iters < 1 || iters > kLidarIters) return -1; // the agent stage is sized for kLidarIters
    const int64_t tasks = lidarTasks(s.A);
    const int64_t per_block = (int64_t)kLidarWaves * iters;
    const int blocks = (int)((tasks + per_block - 1) / per_block);
    return launchByResidency(img, k_lidar, k_lidar_g, dim3(blocks), dim3(kLidarBlock),
                             lidarLdsBytes(sc, img.residency), stream, s, sc, iters);
}

} // namespace mpenv
