// camera.hip — k_camera: the egocentric depth camera (DESIGN.md §2 definition
// 18): per agent a width x height image of depth and label, traced against the
// lidar tree's octant images and the world's capsules from the current state.
// A kernel beside the step, launched behind it while a camera is enabled.
#include "sim_dev.h"

#include "camera.h"
#include "camera_core.h"

namespace mpenv {

static_assert(cameraViewHeight(kStand) == c::kStandHeight - c::kAgentRadius &&
                  cameraViewHeight(kCrouch) == c::kCrouchHeight - c::kAgentRadius &&
                  cameraViewHeight(kProne) == c::kProneHeight - c::kAgentRadius,
              "camera_core.h's view heights are viewHeightD's");

// Lane = pixel.  A wave task is 64 consecutive pixels of one agent's image in
// row-major order (an 8 x 8 image is one task, a 64-wide image one row per
// task): one origin and a narrow solid angle per wave, so its lanes walk
// similar BVH paths, as a forward lidar fan's do; every pixel's arithmetic is
// independent of the grouping.  Blocks and scheduling are k_lidar's: 1024
// threads stage the octant images once, own `iters` x 16 consecutive tasks
// and their 16 waves draw them one at a time from a counter in LDS.  Every
// task is a whole one (width * height is a multiple of 64), so there is no
// tail task: a wave past the last task draws nothing and leaves.
constexpr int kCamBlock = 1024;
constexpr int kCamWaves = kCamBlock / 64;
constexpr int kCamIters = 8;     // compiled maximum of tasks per wave
constexpr int kCamItersAuto = 6; // k_lidar's automatic value: the staging is the same
// The block's agent stage: whole worlds around the agents of its tasks; at one
// task per agent (8 x 8) that is kCamIters x 16 agents and a partial world at
// each end.
constexpr int kCamStageCols = 8;
constexpr int kCamStageMax = kCamIters * kCamWaves + 2 * (2 * kMaxTeamSize - 1) + 2;

// 8 waves per SIMD (64 VGPRs), as k_lidar: the same latency-bound traversal
#define MP_CAMERA_ATTR __attribute__((amdgpu_waves_per_eu(8)))

// Maximum over the lane's DPP row (16 lanes) of non-negative float bit
// patterns compared as signed ints (k_lidar's rowMaxBits16).
__device__ __forceinline__ int camRowMaxBits16(int v)
{
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false));  // quad_perm [1, 0, 3, 2]
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false));  // quad_perm [2, 3, 0, 1]
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x124, 0xF, 0xF, false)); // row_ror:4
    return max(v, __builtin_amdgcn_update_dpp(0, v, 0x128, 0xF, 0xF, false)); // row_ror:8
}

template <class LBVH>
__device__ __forceinline__ void cameraBody(const DevState &S, const SceneDev &sc, const CameraDev &cam, int iters,
                                           char *img)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // the ray tables: sx at 0, sy at kCameraMaxDim
    __shared__ float tab[2 * kCameraMaxDim];
    if (threadIdx.x < 2 * kCameraMaxDim) tab[threadIdx.x] = cam.tab[threadIdx.x];
    const uint32_t N = (uint32_t)S.N, T = (uint32_t)S.T;
    const uint32_t A = (uint32_t)S.A;
    const uint32_t P = (uint32_t)cam.tasksPerAgent, Wd = (uint32_t)cam.width;
    const uint32_t ntasks = A * P;
    // The agents this block's tasks read -- the rays' origins and frames and
    // every capsule of their worlds -- staged in LDS with the BVH, as in
    // k_lidar: whole worlds around the block's task range.
    __shared__ float agentStage[kCamStageCols][kCamStageMax];
    const uint32_t t0 = xcdBlockId() * (uint32_t)iters * kCamWaves;
    const uint32_t t1 = min(ntasks, t0 + (uint32_t)iters * kCamWaves);
    uint32_t s0 = 0, ns = 0;
    if (t0 < t1) {
        const uint32_t a_lo = t0 / P, a_hi = (t1 - 1u) / P + 1u; // <= A
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
            agentStage[7][k] = cameraViewHeight(S.curPose[g]);
        }
    }
    // k_lidar's task counter: wave v starts with task v of the block and draws
    // the next one when it is free
    __shared__ uint32_t nextTask;
    if (threadIdx.x == 0) nextTask = kCamWaves;
    const LBVH bvh = stageBVHOct<LBVH>(LBVH::kStaged ? smem : img, sc); // ends with __syncthreads
    auto draw = [&]() {
        if (iters == 1) return (uint32_t)kCamWaves;
        uint32_t ln, drawn = 0u;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
        if (ln == 0u) drawn = atomicAdd(&nextTask, 1u);
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)drawn);
    };
    for (uint32_t k = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); t0 + k < t1; k = draw()) {
        const uint32_t task = t0 + k; // wave-uniform
        const uint32_t g = task / P, sub = task - g * P;
        const uint32_t ks = g - s0;
        // The lane id is read inside the loop (volatile: not hoisted) and the
        // pixel's indices are formed from it again after the traversal, so that
        // nothing but the ray lives across it (k_lidar, at the same 64 VGPRs).
        uint32_t lane;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
        Vec3 ray_o, dir;
        float tb;
        bool bhit;
        {
            const uint32_t p = sub * 64u + lane;
            const uint32_t r = p / Wd, cc = p - r * Wd;
            const Quat q = quat(agentStage[3][ks], agentStage[4][ks], agentStage[5][ks], agentStage[6][ks]);
            // cameraOrigin with the staged view height
            ray_o = v3(agentStage[0][ks], agentStage[1][ks], agentStage[2][ks]);
            ray_o.z += agentStage[7][ks];
            dir = cameraRayDir(q, tab[cc], tab[kCameraMaxDim + r]);
            // the ray's octant image, walked as k_lidar walks it
            LBVH ob = bvh;
            ob.nodes = reinterpret_cast<const MP_LDS BVHNode *>(reinterpret_cast<const MP_LDS uint4 *>(bvh.nodes) +
                                                                 rayOctant(dir) * sc.numLidarNodes * kOctNodeQ);
            bhit = bvhTraceRayT<false, kOctNodeQ, true, true>(ob, ray_o, dir, tb, kFltMax, 0.f);
        }
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
        const uint32_t w = __umulhi(g, S.nMagic); // g / N (engine.h)
        const uint32_t i = g - w * N;
        const uint32_t kw = w * N - s0; // the world's first agent in the stage
        // The world's capsules, k_lidar's forward-fan cull unchanged (one
        // origin per wave): any point of capsule j lies within r of its
        // vertical axis, so a ray entering it at t has t >= d_xy - r, and a
        // capsule with d_xy - 1.01 r - 1 > max over the wave's rays of the BVH
        // hit t can enter no ray's `t < min_t`.  Lane j < N loads capsule j;
        // the survivors are visited in ascending j.  The agent's own capsule
        // holds the origin (the test returns 0) and is skipped.
        float min_t = bhit ? tb : kFltMax;
        const int rm = camRowMaxBits16(__float_as_int(min_t));
        const float mx = __int_as_float(max(max(__builtin_amdgcn_readlane(rm, 0), __builtin_amdgcn_readlane(rm, 16)),
                                            max(__builtin_amdgcn_readlane(rm, 32), __builtin_amdgcn_readlane(rm, 48))));
        float cx = 0.f, cy = 0.f, cz = 0.f;
        bool keep = false;
        if (lane < N) {
            const uint32_t kc = kw + lane;
            cx = agentStage[0][kc]; cy = agentStage[1][kc]; cz = agentStage[2][kc];
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
        // depth: the lidar's convention; label: 0 miss, 1 wall, 2 teammate, 3 opponent
        float depth = -1.f;
        uint32_t lab = 0u;
        if (hit) {
            depth = fminD(min_t, sc.maxDist);
            lab = ent == -1 ? 1u : ((((uint32_t)ent >= T) == (i >= T)) ? 2u : 3u);
        }
        // Addresses formed after the traversal.  The depth is one coalesced
        // dword store per lane; the labels of a quad's four lanes are gathered
        // into a word (two DPP exchanges) and stored by its first lane: 16
        // dword stores per wave in place of 64 byte stores.
        const int64_t px = (int64_t)g * ((int64_t)P * 64) + (sub * 64u + lane);
        cam.depth[px] = depth;
        uint32_t word = lab << ((lane & 3u) * 8u);
        word |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)word, 0xB1, 0xF, 0xF, false); // quad_perm [1, 0, 3, 2]
        word |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)word, 0x4E, 0xF, 0xF, false); // quad_perm [2, 3, 0, 1]
        if ((lane & 3u) == 0u) reinterpret_cast<uint32_t *>(cam.label)[px >> 2] = word;
    }
}

__global__ void __launch_bounds__(kCamBlock) MP_CAMERA_ATTR k_camera(DevState S, SceneDev sc, CameraDev cam, int iters)
{
    cameraBody<LBVHL>(S, sc, cam, iters, nullptr);
}

__global__ void __launch_bounds__(kCamBlock) MP_CAMERA_ATTR k_camera_g(DevState S, SceneDev sc, CameraDev cam, int iters,
                                                                        SceneImages img)
{
    cameraBody<LBVHG>(S, sc, cam, iters, img.oct);
}

// ============================================================ host side
// Tasks per wave for `tasks` wave tasks: k_lidar's rule (lidarItersFor): ~1024
// blocks before the value grows past 1, kCamItersAuto at most.
static int cameraItersFor(int64_t tasks)
{
    return (int)std::max<int64_t>(1, std::min<int64_t>(kCamItersAuto, tasks / (kCamWaves * 1024)));
}

int launchCamera(const DevState &s, const SceneDev &sc, const SceneImages &img, const CameraDev &cam, void *stream)
{
    const int64_t tasks = s.A * cam.tasksPerAgent;
    if (cam.tasksPerAgent < 1 || tasks >= (int64_t)1 << 31) return -1; // the kernel's task indices are 32-bit
    const int iters = cameraItersFor(tasks);
    const int64_t per_block = (int64_t)kCamWaves * iters;
    const int blocks = (int)((tasks + per_block - 1) / per_block);
    return launchByResidency(img, k_camera, k_camera_g, dim3(blocks), dim3(kCamBlock),
                             lidarLdsBytes(sc, img.residency), stream, s, sc, cam, iters);
}

} // namespace mpenv
