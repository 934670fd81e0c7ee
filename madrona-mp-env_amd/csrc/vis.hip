// vis.hip — k_vis: which opponents each agent sees.
#include "sight_dev.h"

namespace mpenv {

// opponentsWriteVisibilitySystem (sim.cpp:2526-2560) + isAgentVisible
// (utils.cpp:169-271): agent i sees opponent k if any of 4 sample points on
// k (bottom, top, left, right) passes the view tests and the closest hit of
// the ray toward it is k's capsule.
//
// Ray compaction: lane = (agent, opponent); each 64-lane wave holds whole
// agents (floor(64/T) of them).  Phase A tests the sample points (cheap) and
// reserves LDS slots for the candidate rays; phase B traces the compacted
// ray list with every lane of the workgroup, OR-ing hits into per-agent LDS
// masks; phase C writes one mask byte per agent.  Only ~1.5 of the 4 points
// survive the view tests on average, so the dense pass replaces a per-lane
// loop that ran at roughly a third of the wave's lanes.
constexpr int kVisMaxRays = kBlock * 4;

// k_vis stages its block's agents with their worlds' whole rosters (the
// opponents the block's lanes test and every capsule a ray may meet) in LDS
// after the BVH image: 4 waves x floor(64/T) agents plus up to N-1 agents of
// the partial first and last worlds.  Columns: px, py, pz, view height,
// aim quaternion (w, x, y, z), alive.
constexpr int kVisStageCols = 9;
__host__ __device__ __forceinline__ int visStageAgents(int T, int N) { return (kBlock / 64) * (64 / T) + 2 * (N - 1); }

template <class LBVH>
__device__ __forceinline__ void visBody(const DevState &S, const SceneDev &sc, char *img)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ uint16_t rays[kVisMaxRays];  // (lane << 2) | point
    __shared__ uint16_t rays2[kVisMaxRays]; // phase B2: indices into rays
    __shared__ uint32_t masks[kBlock]; // per agent of the block (<= 4 waves x 64/T)
    __shared__ uint32_t nrays, nrays2;
    if (threadIdx.x == 0) {
        nrays = 0;
        nrays2 = 0;
    }
    masks[threadIdx.x] = 0;
    const int T = S.T, N = S.N;
    const int apw = 64 / T;
    const int wl = threadIdx.x & 63;
    const int64_t wave = ((int64_t)xcdBlockId() * blockDim.x + threadIdx.x) >> 6;
    const int64_t agent0 = (((int64_t)xcdBlockId() * blockDim.x) >> 6) * apw; // first agent of the block
    const int nsMax = visStageAgents(T, N);
    float *st = (float *)(smem + (LBVH::kStaged ? CollisionImage { sc.numNodes, sc.numVerts }.bytes() : 0));
    const int64_t s0 = (agent0 / N) * N;
    {
        const int64_t a_hi = min(S.A, agent0 + (int64_t)(kBlock / 64) * apw);
        const int ns = agent0 < a_hi ? (int)(((a_hi - 1) / N + 1) * N - s0) : 0;
        for (int k = threadIdx.x; k < ns; k += kBlock) {
            const int64_t g = s0 + k;
            st[0 * nsMax + k] = S.px[g];
            st[1 * nsMax + k] = S.py[g];
            st[2 * nsMax + k] = S.pz[g];
            st[3 * nsMax + k] = viewHeightD(S.curPose[g]);
            st[4 * nsMax + k] = S.aw[g];
            st[5 * nsMax + k] = S.ax[g];
            st[6 * nsMax + k] = S.ay[g];
            st[7 * nsMax + k] = S.az[g];
            st[8 * nsMax + k] = S.alive[g];
        }
    }
    // The collision tree, as isAgentVisible walks it (the reference has one
    // tree): which triangles a traversal reaches depends on the tree for rays
    // along a zero-margin child box face, so another tree can answer
    // differently (DESIGN.md section 2 definition 4).  Barrier.
    const LBVH bvh = stageBVH<LBVH>(LBVH::kStaged ? smem : img, sc);
    auto sPos = [&](int64_t g) {
        const int l = (int)(g - s0);
        return v3(st[0 * nsMax + l], st[1 * nsMax + l], st[2 * nsMax + l]);
    };
    auto sAim = [&](int64_t g) {
        const int l = (int)(g - s0);
        return quat(st[4 * nsMax + l], st[5 * nsMax + l], st[6 * nsMax + l], st[7 * nsMax + l]);
    };
    auto sView = [&](int64_t g) { return st[3 * nsMax + (int)(g - s0)]; };
    auto sAlive = [&](int64_t g) { return st[8 * nsMax + (int)(g - s0)]; };
    // visSamplePointD from the stage
    auto sSample = [&](int64_t gt, Vec3 delta_right, int p) {
        Vec3 pt = sPos(gt);
        pt.z += p == 0 ? c::kAgentRadius : sView(gt);
        if (p == 2) pt = pt - delta_right;
        if (p == 3) pt = pt + delta_right;
        return pt;
    };

    // ---- phase A: view tests, reserve ray slots
    {
        const int64_t g = wave * apw + wl / T;
        const int k = wl % T;
        const bool valid = wl < apw * T && g < S.A;
        uint32_t cand = 0;
        if (valid) {
            const int w = (int)(g / N);
            const int i = (int)(g - (int64_t)w * N);
            const int64_t gt = (int64_t)w * N + ((i / T) ^ 1) * T + k;
            if (sAlive(g) != 0.f && sAlive(gt) != 0.f) {
                Vec3 org = sPos(g);
                org.z += sView(g);
                const Quat aim_rot = sAim(g);
                const Quat inv_rot = qinv(aim_rot);
                const Vec3 delta_right = rotateVec(aim_rot, kRight) * 0.9f * c::kAgentRadius;
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    Vec3 to_test = sSample(gt, delta_right, p) - org;
                    Vec3 view = rotateVec(inv_rot, to_test);
                    if (view.y <= 0.f) continue;
                    if (!inFrustumD(sc, view)) continue;
                    if (length(to_test) < c::kAgentRadius) continue;
                    cand |= 1u << p;
                }
            }
        }
        const int nc = __popc(cand);
        if (S.stats) {
            uint32_t pair = 0;
            if (valid && sAlive(g) != 0.f) {
                const int64_t gt2 = (g / N) * N + (((int)(g % N) / T) ^ 1) * T + k;
                pair = sAlive(gt2) != 0.f ? 1u : 0u;
            }
            statAdd(S.stats + kStatLosPairs, pair);
            statAdd(S.stats + kStatLosRays, (uint32_t)nc);
        }
        // Ray-slot reservation: the wave's exclusive prefix sum of its
        // lanes' candidate counts (4 ballots of one bit each, mbcnt), one
        // LDS atomic per wave for the base.
        uint32_t before = 0, wtotal = 0;
#pragma unroll
        for (int bit = 0; bit < 3; bit++) {
            const uint64_t m = __ballot((nc >> bit) & 1);
            before += (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)) << bit;
            wtotal += (uint32_t)__popcll(m) << bit;
        }
        uint32_t base = 0;
        if (wl == 0 && wtotal) base = atomicAdd(&nrays, wtotal);
        base = __shfl(base, 0);
        if (nc) {
            uint32_t slot = base + before;
            const uint16_t lane_id = (uint16_t)(threadIdx.x << 2);
            for (int p = 0; p < 4; p++)
                if (cand & (1u << p)) rays[slot++] = (uint16_t)(lane_id | p);
        }
    }
    __syncthreads();

    // ---- phase B: the compacted rays.  B1 decides what needs no traversal
    // (target capsule missed, occluder hint hit); the rest are compacted
    // again so B2's traversals run in dense waves (a wave of mixed rays
    // otherwise idles all but its few traversing lanes).
    const uint32_t total = nrays;
    const uint32_t numTris = (uint32_t)(sc.numVerts / 3);
    // the occluder hint stores triangle ids as u16 with 0xffff = none: off
    // for scenes of 65,535 triangles or more
    const bool hints = numTris < 0xffffu;
    auto rayOf = [&](uint32_t r, int64_t &g, int &k, int &p, int64_t &g0, int &target, Vec3 &org, Vec3 &dir) {
        const uint32_t d = rays[r];
        const int lane = (int)(d >> 2);
        p = (int)(d & 3);
        const int lwl = lane & 63;
        g = ((((int64_t)xcdBlockId() * blockDim.x + lane) >> 6) * apw) + lwl / T;
        k = lwl % T;
        const int w = (int)(g / N);
        const int i = (int)(g - (int64_t)w * N);
        g0 = (int64_t)w * N;
        target = ((i / T) ^ 1) * T + k;
        org = sPos(g);
        org.z += sView(g);
        const Quat aim_rot = sAim(g);
        const Vec3 delta_right = rotateVec(aim_rot, kRight) * 0.9f * c::kAgentRadius;
        Vec3 to_test = sSample(g0 + target, delta_right, p) - org;
        const float len = length(to_test);
        dir = to_test / len;
    };
    for (uint32_t r = threadIdx.x; r < total; r += kBlock) {
        int64_t g, g0;
        int k, p, target;
        Vec3 org, dir;
        rayOf(r, g, k, p, g0, target, org, dir);
        float t_c;
        const int l0 = (int)(g0 - s0);
        auto capsule = [&](int j) { return v3(st[0 * nsMax + l0 + j], st[1 * nsMax + l0 + j], st[2 * nsMax + l0 + j]); };
        if (!visibleQuickD(bvh, capsule, org, dir, target,
                           hints ? S.visOcc + (g * T + k) * 4 + p : nullptr, numTris, t_c))
            rays2[atomicAdd(&nrays2, 1u)] = (uint16_t)r;
    }
    __syncthreads();
    const uint32_t total2 = nrays2;
    if (S.stats && threadIdx.x == 0) atomicAdd(S.stats + kStatLosTraced, (unsigned long long)total2);
    for (uint32_t q = threadIdx.x; q < total2; q += kBlock) {
        int64_t g, g0;
        int k, p, target;
        Vec3 org, dir;
        rayOf(rays2[q], g, k, p, g0, target, org, dir);
        // t_c again (the same bits as in B1)
        const int l0 = (int)(g0 - s0);
        auto capsule = [&](int j) { return v3(st[0 * nsMax + l0 + j], st[1 * nsMax + l0 + j], st[2 * nsMax + l0 + j]); };
        Vec3 ct = capsule(target);
        ct.z += kCapsuleRadius;
        const float t_c = intersectRayZOriginCapsule(org - ct, dir, kCapsuleRadius, kCapsuleSegment);
        const bool seen = visibleFullD(bvh, capsule, N, org, dir, target, t_c,
                                       hints ? S.visOcc + (g * T + k) * 4 + p : nullptr);
        if (seen) atomicOr(&masks[(int)(g - agent0)], 1u << k);
        if (S.stats) statAdd(S.stats + kStatLosSeen, seen ? 1u : 0u);
    }
    __syncthreads();

    // ---- phase C: one byte per agent
    {
        const int64_t g = wave * apw + wl / T;
        const bool valid = wl < apw * T && g < S.A;
        if (valid && wl % T == 0) S.visMask[g] = (uint8_t)masks[(int)(g - agent0)];
    }
}

__global__ void __launch_bounds__(kBlock) k_vis(DevState S, SceneDev sc)
{
    visBody<LBVHL>(S, sc, nullptr);
}

__global__ void __launch_bounds__(kBlock) k_vis_g(DevState S, SceneDev sc, SceneImages img)
{
    visBody<LBVHG>(S, sc, img.sphere);
}

// ============================================================ host side
size_t visLdsBytes(const SceneDev &sc, int32_t residency, int T)
{
    size_t stage = 0;
    for (int t = T > 0 ? T : 1; t <= (T > 0 ? T : kMaxTeamSize); t++)
        stage = std::max(stage, (size_t)kVisStageCols * 4 * visStageAgents(t, 2 * t));
    return (residency == kResidencyGlobal ? 0 : bvhLdsBytes(sc)) + stage;
}

int launchVisibility(const DevState &s, const SceneDev &sc, const SceneImages &img, void *stream)
{
    const int64_t waves = (s.A + (64 / s.T) - 1) / (64 / s.T);
    const int blocks = (int)((waves * 64 + kBlock - 1) / kBlock);
    return launchByResidency(img, k_vis, k_vis_g, dim3(blocks), dim3(kBlock), visLdsBytes(sc, img.residency, s.T),
                             stream, s, sc);
}

} // namespace mpenv
