// hooks.hip — debug and test hooks: caller-ray traces, geometry queries
// through the step kernels' own device functions, and the debug gather.
#include "casts_dev.h"

namespace mpenv {

// Which image a hook's kernel walks (the geometry-query hook: the image of the
// kernel each mode stands in for), and the dynamic LDS it asks for.
enum class HookImage { Collision, Sphere, Oct };

constexpr HookImage geomImage(int mode)
{
    return mode == MPENV_GEOM_LIDAR_RAY ? HookImage::Oct
           : mode == MPENV_GEOM_WORLD_RAY || mode == MPENV_GEOM_SIGHT ? HookImage::Collision : HookImage::Sphere;
}

static size_t hookLdsBytes(const SceneDev &sc, int32_t residency, HookImage image)
{
    if (residency == kResidencyGlobal) return 0;
    return image == HookImage::Oct ? bvhLdsBytesOct(sc) : image == HookImage::Sphere ? bvhLdsBytesSphere(sc) : bvhLdsBytes(sc);
}

// Debug/test hook: closest-hit BVH queries for caller rays (mode 0 = the
// traversal inlined into the step kernels, 1 = its out-of-line copy).
template <class LBVH>
__device__ __forceinline__ void traceRaysBody(const SceneDev &sc, const float *o, const float *d, int n, int mode,
                                              float *t_out, int32_t *hit_out, char *img)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const LBVH bvh = stageBVH<LBVH>(LBVH::kStaged ? smem : img, sc);
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const Vec3 org = v3(o[3 * r], o[3 * r + 1], o[3 * r + 2]);
    const Vec3 dir = v3(d[3 * r], d[3 * r + 1], d[3 * r + 2]);
    float t = 0.f;
    bool hit;
    if (mode == 0) {
        hit = bvhTraceRayD(bvh, org, dir, t); // inlined, as in the step kernels
    } else {
        RayHitD h = bvhTraceRayExactD(bvh, org, dir);
        hit = h.hit != 0;
        t = h.t;
    }
    t_out[r] = hit ? t : 0.f;
    hit_out[r] = hit ? 1 : 0;
}

__global__ void __launch_bounds__(kBlock) k_trace_rays(SceneDev sc, const float *o, const float *d, int n, int mode,
                                                       float *t_out, int32_t *hit_out)
{
    traceRaysBody<LBVHL>(sc, o, d, n, mode, t_out, hit_out, nullptr);
}

__global__ void __launch_bounds__(kBlock) k_trace_rays_g(SceneDev sc, const float *o, const float *d, int n, int mode,
                                                         float *t_out, int32_t *hit_out, SceneImages img)
{
    traceRaysBody<LBVHG>(sc, o, d, n, mode, t_out, hit_out, img.sphere);
}

int launchTraceRays(const SceneDev &sc, const SceneImages &img, const float *o, const float *d, int n, int mode,
                    float *t, int32_t *hit, void *stream)
{
    if (n <= 0) return 0;
    return launchByResidency(img, k_trace_rays, k_trace_rays_g, dim3((n + kBlock - 1) / kBlock), dim3(kBlock),
                             hookLdsBytes(sc, img.residency, HookImage::Collision), stream, sc, o, d, n, mode, t, hit);
}

// Test hook (mpenv_debug_geom_queries, include/mpenv.h): one geometry query
// per thread through the step kernels' own device functions, on the image
// (LDS- or global-resident, as the step kernels' own) of the kernel each mode
// stands in for (k_lidar / k_sim / k_vis / k_move).
// The functions are force-inlined, so this is a second compilation of them:
// it checks their shortcut arguments on chosen inputs, not the step kernels'
// code generation (whole-step parity covers that).
template <int kMode, class LBVH>
__device__ __forceinline__ void geomQueriesBody(const SceneDev &sc, const mpenv_geom_queries &q, int n,
                                                const SceneImages &img)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    LBVH bvh;
    if constexpr (geomImage(kMode) == HookImage::Oct) bvh = stageBVHOct<LBVH>(LBVH::kStaged ? smem : img.oct, sc);
    else if constexpr (geomImage(kMode) == HookImage::Collision) bvh = stageBVH<LBVH>(LBVH::kStaged ? smem : img.sphere, sc);
    else bvh = stageBVHSphere<LBVH>(LBVH::kStaged ? smem : img.sphere, sc);
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const Vec3 org = v3(q.o[3 * r], q.o[3 * r + 1], q.o[3 * r + 2]);
    const Vec3 dir = v3(q.d[3 * r], q.d[3 * r + 1], q.d[3 * r + 2]);
    const int N = q.num_caps;
    if constexpr (kMode == MPENV_GEOM_LIDAR_RAY) {
        // as k_lidar forms `ob`
        LBVH ob = bvh;
        ob.nodes = reinterpret_cast<const MP_LDS BVHNode *>(reinterpret_cast<const MP_LDS uint4 *>(bvh.nodes) +
                                                             rayOctant(dir) * sc.numLidarNodes * kOctNodeQ);
        float tb;
        const bool hit = bvhTraceRayT<false, kOctNodeQ, true, true>(ob, org, dir, tb, kFltMax, 0.f);
        q.t[r] = tb;
        q.i0[r] = hit ? 1 : 0;
    } else if constexpr (kMode == MPENV_GEOM_WORLD_RAY) {
        float cx[12], cy[12], cz[12]; // the query's world as position columns
        for (int j = 0; j < N; j++) {
            const float *cp = q.caps + ((size_t)r * N + j) * 3;
            cx[j] = cp[0]; cy[j] = cp[1]; cz[j] = cp[2];
        }
        const WorldHit h = traceWorldD(bvh, cx, cy, cz, 0, N, org, dir, q.sel[r]);
        q.i0[r] = h.hit ? 1 : 0;
        q.t[r] = h.t;
        q.i1[r] = h.entity;
    } else if constexpr (kMode == MPENV_GEOM_SIGHT) {
        const int target = q.sel[r];
        bool seen;
        if (q.sub == 0) {
            // k_vis phase B: B1 on every ray, B2 on the unresolved ones
            const uint32_t numTris = (uint32_t)(sc.numVerts / 3);
            const bool hints = numTris < 0xffffu;
            auto capsule = [&](int j) {
                const float *cp = q.caps + ((size_t)r * N + j) * 3;
                return v3(cp[0], cp[1], cp[2]);
            };
            float t_c;
            seen = false;
            if (!visibleQuickD(bvh, capsule, org, dir, target, hints ? q.hint + r : nullptr, numTris, t_c))
                seen = visibleFullD(bvh, capsule, N, org, dir, target, t_c, hints ? q.hint + r : nullptr);
        } else {
            float cx[12], cy[12], cz[12];
            for (int j = 0; j < N; j++) {
                const float *cp = q.caps + ((size_t)r * N + j) * 3;
                cx[j] = cp[0]; cy[j] = cp[1]; cz[j] = cp[2];
            }
            seen = visibleRayD(bvh, cx, cy, cz, 0, N, org, dir, target);
        }
        q.i0[r] = seen ? 1 : 0;
    } else if constexpr (kMode == MPENV_GEOM_CASTS) {
        if (q.sub == 2) {
            SphereHit h0, h1;
            h1.t = kFltMax;
            h1.n = v3(0.f, 0.f, 0.f);
            castNear2D(bvh, sc, org, q.z1[r], dir, q.bound[r], q.sel[r] != 0, h0, h1);
            q.t[2 * r] = h0.t;
            q.t[2 * r + 1] = h1.t;
            float *np = q.normal + (size_t)r * 6;
            np[0] = h0.n.x; np[1] = h0.n.y; np[2] = h0.n.z;
            np[3] = h1.n.x; np[4] = h1.n.y; np[5] = h1.n.z;
        } else if (q.sub == 3) {
            q.t[r] = castFirstNearD(bvh, sc, org, dir, q.bound[r]);
        } else {
            const SphereHit h = q.sub == 0 ? bvhSphereCastD(bvh, org, dir, kSphereR)
                                           : castNearD(bvh, sc, org, dir, q.bound[r]);
            q.t[r] = h.t;
            q.normal[3 * r] = h.n.x; q.normal[3 * r + 1] = h.n.y; q.normal[3 * r + 2] = h.n.z;
        }
    } else {
        // applyVelocityD's call: lanes that left k_move early are gone, the
        // rest call with or without `need`
        const int flags = q.sel[r];
        if (!(flags & 1)) return;
        float hd4[4];
        for (int k = 0; k < 4; k++) hd4[k] = q.t[4 * r + k];
        stuckCastsD(bvh, (flags & 2) != 0, org, dir, q.bound[r], hd4);
        for (int k = 0; k < 4; k++) q.t[4 * r + k] = hd4[k];
    }
}

template <int kMode>
__global__ void __launch_bounds__(kBlock) k_geom_queries(SceneDev sc, mpenv_geom_queries q, int n)
{
    geomQueriesBody<kMode, LBVHL>(sc, q, n, SceneImages {});
}

template <int kMode>
__global__ void __launch_bounds__(kBlock) k_geom_queries_g(SceneDev sc, mpenv_geom_queries q, int n, SceneImages img)
{
    geomQueriesBody<kMode, LBVHG>(sc, q, n, img);
}

template <int kMode>
static int launchGeomMode(const SceneDev &sc, const SceneImages &img, int n, const mpenv_geom_queries &q, void *stream)
{
    return launchByResidency(img, k_geom_queries<kMode>, k_geom_queries_g<kMode>, dim3((n + kBlock - 1) / kBlock),
                             dim3(kBlock), hookLdsBytes(sc, img.residency, geomImage(kMode)), stream, sc, q, n);
}

int launchGeomQueries(const SceneDev &sc, const SceneImages &img, int mode, int n, const mpenv_geom_queries &q,
                      void *stream)
{
    if (n <= 0) return 0;
    switch (mode) {
    case MPENV_GEOM_LIDAR_RAY: return launchGeomMode<MPENV_GEOM_LIDAR_RAY>(sc, img, n, q, stream);
    case MPENV_GEOM_WORLD_RAY: return launchGeomMode<MPENV_GEOM_WORLD_RAY>(sc, img, n, q, stream);
    case MPENV_GEOM_SIGHT: return launchGeomMode<MPENV_GEOM_SIGHT>(sc, img, n, q, stream);
    case MPENV_GEOM_CASTS: return launchGeomMode<MPENV_GEOM_CASTS>(sc, img, n, q, stream);
    case MPENV_GEOM_STUCK: return launchGeomMode<MPENV_GEOM_STUCK>(sc, img, n, q, stream);
    default: return -1;
    }
}

// Debug gather of internal state into the MPENV_EXPORT_DEBUG_* layouts.
__global__ void __launch_bounds__(256) k_debug(DevState S, float *af, int32_t *ai, int32_t *wi, float *wf,
                                               uint32_t *explore, float *crumbs)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < S.A) {
        const int64_t g = t;
        float *f = &af[g * MPENV_DBG_AF_COUNT];
        f[0] = S.px[g]; f[1] = S.py[g]; f[2] = S.pz[g];
        f[3] = S.vx[g]; f[4] = S.vy[g]; f[5] = S.vz[g];
        f[6] = S.rw[g]; f[7] = S.rx[g]; f[8] = S.ry[g]; f[9] = S.rz[g];
        f[10] = S.ayaw[g]; f[11] = S.apitch[g];
        f[12] = S.aw[g]; f[13] = S.ax[g]; f[14] = S.ay[g]; f[15] = S.az[g];
        f[16] = S.maxVel[g]; f[17] = S.minDistZone[g]; f[18] = S.firedT[g]; f[19] = S.bcPenalty[g];
        f[20] = S.sx[g]; f[21] = S.sy[g]; f[22] = S.sz[g];
        f[23] = S.minDistSub[g];
        int32_t *n = &ai[g * MPENV_DBG_AI_COUNT];
        n[0] = S.curPose[g]; n[1] = S.tgtPose[g]; n[2] = S.transRem[g];
        n[3] = S.rngA[g]; n[4] = S.rngB[g]; n[5] = S.rngCtr[g];
        n[6] = S.landedOn[g]; n[7] = S.respawnSteps[g]; n[8] = S.autohealSteps[g];
        n[9] = S.flags[g] & 63;
        n[10] = S.wasShot[g]; n[11] = S.weapon[g]; n[12] = S.bcLast[g]; n[13] = S.bcSteps[g];
        n[14] = S.visMask[g];
        n[15] = S.newCells[g];
        if (explore) {
            // 1 = visited in the agent's current episode (the reference's
            // tag == curEpisodeIdx), 0 otherwise
            const bool cur = S.exploreEp[g] == S.episode[g / S.N];
            const int ct = S.exploreTile[g];
            const uint64_t cw = (uint64_t)(uint32_t)S.exploreLo[g] | ((uint64_t)(uint32_t)S.exploreHi[g] << 32);
            for (int k = 0; k < kGridCells; k++) {
                const int cy = k / kGridW, cx = k - cy * kGridW;
                const int t = exploreTileD(cx, cy);
                const uint64_t word = t == ct ? cw : S.exploreBits[g * kExploreTiles + t];
                explore[g * kGridCells + k] = cur ? (uint32_t)((word >> exploreBitD(cx, cy)) & 1ull) : 0u;
            }
        }
    }
    if (t < S.W) {
        const int w = (int)t;
        int32_t *n = &wi[(int64_t)w * MPENV_DBG_WI_COUNT];
        n[0] = S.teamA[w]; n[1] = S.curStep[w]; n[2] = S.finished[w]; n[3] = S.curZone[w];
        n[4] = S.controlling[w]; n[5] = S.contested[w]; n[6] = S.captured[w]; n[7] = S.earned[w];
        n[8] = S.zoneSteps[w]; n[9] = S.stepsUntilPoint[w]; n[10] = S.episode[w]; n[11] = S.episodeCounter[w];
        n[12] = S.wRngA[w]; n[13] = S.wRngB[w]; n[14] = S.wRngCtr[w]; n[15] = S.numCrumbs[w];
        n[16] = S.filtAct0[w]; n[17] = S.filtAct1[w]; n[18] = S.filtMatched0[w]; n[19] = S.filtMatched1[w];
        n[20] = S.crumbOverflow[w];
        n[21] = S.subState[w];
        float *f = &wf[(int64_t)w * MPENV_DBG_WF_COUNT];
        f[0] = S.teamRew0[w]; f[1] = S.teamRew1[w]; f[2] = S.goalMin0[w]; f[3] = S.goalMin1[w];
        f[4] = S.goalTeam0[w]; f[5] = S.goalTeam1[w];
        float *cdst = &crumbs[(int64_t)w * kMaxCrumbs * 8];
        const float4 *cr = crumbPtr(S, w);
        const int nc = S.numCrumbs[w];
        for (int k = 0; k < kMaxCrumbs; k++) {
            float *e = &cdst[k * 8];
            if (k < nc) {
                float4 p = cr[2 * k], meta = cr[2 * k + 1];
                e[0] = p.x; e[1] = p.y; e[2] = p.z; e[3] = p.w;
                e[4] = meta.x; e[5] = meta.y; e[6] = (float)__float_as_int(meta.z); e[7] = 1.f;
            } else {
                for (int q = 0; q < 8; q++) e[q] = 0.f;
            }
        }
    }
}

// ============================================================ host side
int launchDebugGather(const DevState &s, float *af, int32_t *ai, int32_t *wi, float *wf, uint32_t *explore,
                      float *crumbs, void *stream)
{
    const int64_t n = s.A > s.W ? s.A : s.W;
    hipLaunchKernelGGL(k_debug, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, s, af, ai, wi,
                       wf, explore, crumbs);
    return check(hipGetLastError());
}

} // namespace mpenv
