// casts_dev.h — k_move's sphere-cast shortcuts, shared with the geometry-query
// test hook (hooks.hip), which runs the same functions query by query.
#pragma once
#include "sim_dev.h"

namespace mpenv {

__device__ __forceinline__ Vec3 rotate2DD(Vec3 dir, float radians) // sim.cpp:874-879
{
    float cc = cosf_(radians);
    float s = sinf_(radians);
    return v3(cc * dir.x - s * dir.y, s * dir.x + cc * dir.y, 0);
}

// Distance-bounded sphere casts (k_move).  MeshBVH::sphereCast prunes boxes
// beyond its current hit, so with t_max = B it visits the same boxes in the
// same order as the unbounded cast minus those entered beyond B, and
// returns the same hit and normal whenever the unbounded cast's hit is
// nearer than B -- except through the vertex-test quirk (scene.h
// quirkGrid): testVert tests the ray 2o + t·d against a sphere of radius r
// around each vertex, so a visited triangle with a vertex within r of that
// ray at some t < B returns t (0 when 2o itself is inside) although the
// geometry is far away; a bounded cast may never visit that triangle.  A
// bounded cast is therefore only used when every grid cell under the xy
// path 2o .. 2o + B·d is clear (each clear cell is farther than r + 2 from
// every vertex); otherwise, and where the caller needs more than "hit
// nearer than B or not", the full cast runs.  Vertical casts have a
// one-cell path.  DESIGN.md §2.
// Bound = the largest distance the caller compares a hit with + this slack
// (a bounded miss then reads as a hit that far away, well past every
// comparison, whatever the rounding).
constexpr float kCastSlack = 4.f;

__device__ __forceinline__ bool castQuirkFreeD(const SceneDev &sc, Vec3 o)
{
    const float fx = ((o.x + o.x) - sc.qgMinX) * sc.qgInvCell;
    const float fy = ((o.y + o.y) - sc.qgMinY) * sc.qgInvCell;
    if (!(fx >= 0.f && fx < (float)sc.qgW && fy >= 0.f && fy < (float)sc.qgH)) return true;
    const uint32_t bit = (uint32_t)(int)fy * (uint32_t)sc.qgW + (uint32_t)(int)fx;
    return !((sc.quirkGrid[bit >> 5] >> (bit & 31)) & 1u);
}

// Every cell of the xy bounding box of the segment 2o .. 2o + B·d is clear
// (cells outside the grid are clear by construction: the grid reaches
// r + margin + one cell beyond every vertex).
__device__ __forceinline__ bool castPathQuirkFreeD(const SceneDev &sc, Vec3 o, Vec3 d, float B)
{
    const float px = o.x + o.x, py = o.y + o.y;
    const float qx = px + d.x * B, qy = py + d.y * B;
    const int x0 = max((int)floorf((fminf(px, qx) - sc.qgMinX) * sc.qgInvCell), 0);
    const int x1 = min((int)floorf((fmaxf(px, qx) - sc.qgMinX) * sc.qgInvCell), sc.qgW - 1);
    const int y0 = max((int)floorf((fminf(py, qy) - sc.qgMinY) * sc.qgInvCell), 0);
    const int y1 = min((int)floorf((fmaxf(py, qy) - sc.qgMinY) * sc.qgInvCell), sc.qgH - 1);
    for (int y = y0; y <= y1; y++)
        for (int x = x0; x <= x1; x++) {
            const uint32_t bit = (uint32_t)y * (uint32_t)sc.qgW + (uint32_t)x;
            if ((sc.quirkGrid[bit >> 5] >> (bit & 31)) & 1u) return false;
        }
    return true;
}

// The cast's hit if nearer than `near_b`, else t = kFltMax: for callers to
// which every hit at or beyond near_b acts like no hit.  Horizontal d.
template <class LBVH>
__device__ __forceinline__ SphereHit castNearD(const LBVH &bvh, const SceneDev &sc, Vec3 o, Vec3 d, float near_b)
{
    if (!castPathQuirkFreeD(sc, o, d, near_b)) return bvhSphereCastD(bvh, o, d, kSphereR);
    SphereHit h = bvhSphereCastD(bvh, o, d, kSphereR, near_b);
    if (!(h.t < near_b)) h.t = kFltMax;
    return h;
}

// castNearD for the low cast from o and, when act1, the high cast from
// (o.x, o.y, z1): one traversal (bvhSphereCast2D), the same results.  The
// path guard depends on o.xy, d and near_b only, so both casts take the
// same branch.
template <class LBVH>
__device__ __forceinline__ void castNear2D(const LBVH &bvh, const SceneDev &sc, Vec3 o, float z1, Vec3 d,
                                           float near_b, bool act1, SphereHit &h0, SphereHit &h1)
{
    if (!castPathQuirkFreeD(sc, o, d, near_b)) {
        bvhSphereCast2D(bvh, o, z1, d, kSphereR, kFltMax, act1, h0, h1);
        return;
    }
    bvhSphereCast2D(bvh, o, z1, d, kSphereR, near_b, act1, h0, h1);
    if (!(h0.t < near_b)) h0.t = kFltMax;
    if (act1 && !(h1.t < near_b)) h1.t = kFltMax;
}

// The full cast's t, searched within near_b first.  Vertical d only (the
// path guard is the cell of 2o).
template <class LBVH>
__device__ __forceinline__ float castFirstNearD(const LBVH &bvh, const SceneDev &sc, Vec3 o, Vec3 d, float near_b)
{
    if (castQuirkFreeD(sc, o)) {
        const float t = bvhSphereCastD(bvh, o, d, kSphereR, near_b).t;
        if (t < near_b) return t;
    }
    return bvhSphereCastD(bvh, o, d, kSphereR).t;
}

// Index of the n-th set bit (0-based) of m; m has more than n set bits.
__device__ __forceinline__ int nthSetBitD(uint64_t m, int n)
{
    int pos = 0;
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
        const uint64_t low = m & ((1ull << w) - 1ull);
        const int c = __popcll(low);
        if (n >= c) {
            n -= c;
            m >>= w;
            pos += w;
        } else {
            m = low;
        }
    }
    return pos;
}

// The "stuck" fallback's four horizontal casts (sim.cpp:962-984), for the
// lanes of the wave with `need` set: their 4·k casts are dealt one per
// active lane across the wave (rounds of as many casts as the wave has
// active lanes) instead of four in a row on the owning lane -- a wave holding
// one stuck agent runs one cast's time, not four.  Each cast is the same
// function of the same owner inputs (x, v_norm, low_check shuffled from the
// owner), so hd4 is bit-identical to the serial loop's.  Called by every
// active lane of the wave; on small batches k_move runs 8-32 agents per
// wave (launchMove), and round 6 deals over those lanes too (rounds 4-5 fell
// back to the serial loop on any partial wave, i.e. always below C3).
template <class LBVH>
__device__ __forceinline__ void stuckCastsD(const LBVH &bvh, bool need, Vec3 x, Vec3 v_norm, float low_check,
                                            float hd4[4])
{
    const float r = c::kAgentRadius;
    const uint64_t act = __ballot(1);
    const uint64_t m = __ballot(need);
    if (m == 0ull) return;
    const int na = __popcll(act);
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int arank = __popcll(act & ((1ull << lane) - 1ull)); // this lane's index among the active lanes
    const int rank = __popcll(m & ((1ull << lane) - 1ull));    // owner's index among the stuck lanes
    const int tasks = 4 * __popcll(m);
    for (int base = 0; base < tasks; base += na) {
        const int t = base + arank;
        const int owner = nthSetBitD(m, min(t, tasks - 1) >> 2);
        const float ox = __shfl(x.x, owner), oy = __shfl(x.y, owner), oz = __shfl(x.z, owner);
        const float vx = __shfl(v_norm.x, owner), vy = __shfl(v_norm.y, owner), vz = __shfl(v_norm.z, owner);
        const float lc = __shfl(low_check, owner);
        float hd = 0.f;
        if (t < tasks) {
            const Vec3 dv = rotate2DD(v3(vx, vy, vz), (float)(t & 3) * 3.14159f * 0.5f);
            Vec3 ray_o = v3(ox, oy, oz) - dv * r * 2.0f;
            ray_o.z += lc;
            hd = bvhSphereCastD(bvh, ray_o, dv, r).t;
        }
#pragma unroll
        for (int dir = 0; dir < 4; dir++) {
            const int tt = 4 * rank + dir;
            // the active lane that ran task tt this round (any lane when none did)
            const int src = nthSetBitD(act, min(max(tt - base, 0), na - 1));
            const float got = __shfl(hd, src);
            if (need && tt >= base && tt < base + na) hd4[dir] = got;
        }
    }
}

} // namespace mpenv
