// nav_dev.h — the navmesh queries of the scripted bots (k_move's planAStarD)
// and of the scene-upload kernels, and the frame of a rotated box.
//
// navTriCenterD, nearestNavTriD and pathfindToPointD are not inline (their
// inlining is the compiler's choice, as it was in one file): more than one unit
// may define them only because device code is compiled without -fgpu-rdc, each
// unit its own code object, and the host side emits nothing for them.
#pragma once
#include "sim_dev.h"

namespace mpenv {

// ---- scripted bots: NavUtils (sim.cpp:4958-5037) + planAStarAISystem
// (sim.cpp:5041-5172).  The triangle loops index the navmesh uniformly
// across the wave, so its vertices come in as scalar loads.
__device__ __forceinline__ Vec3 navVertD(const SceneDev &sc, int tri, int k)
{
    const float *p = sc.navTris + 9 * tri + 3 * k;
    return v3(p[0], p[1], p[2]);
}

__device__ Vec3 navTriCenterD(const SceneDev &sc, int tri)
{
    Vec3 c = v3(0.f, 0.f, 0.f);
    for (int k = 0; k < 3; k++) c = c + navVertD(sc, tri, k) / 3.0f;
    return c;
}

// NearestNavTri (sim.cpp:4975-5010): first containing triangle (xy winding
// test), else the candidate kept by the reference's distance bookkeeping.
__device__ int nearestNavTriD(const SceneDev &sc, Vec3 pos)
{
    float closest = kFltMax;
    int closest_idx = -1;
    for (int tri = 0; tri < sc.numNavTris; tri++) {
        bool contained = true;
        bool gtz = false;
        for (int k = 0; k < 3; k++) {
            const Vec3 v1 = navVertD(sc, tri, k);
            const Vec3 v2 = navVertD(sc, tri, k == 2 ? 0 : k + 1);
            const Vec3 e = v2 - v1;
            const Vec3 vp = pos - v1;
            const Vec3 c = cross(e, vp);
            if ((c.z > 0.0f) != gtz && k > 0) contained = false;
            gtz = c.z > 0.0f;
            float distsq = length2(v1 - pos);
            if (distsq < closest) {
                const float dir = dot(e, vp);
                const Vec3 perp = vp * (-dir / dot(e, e)) + e;
                distsq = dot(perp, perp);
                if (distsq < closest) {
                    closest = fabs_(c.z);
                    closest_idx = tri;
                }
            }
        }
        if (contained) return tri;
    }
    return closest_idx;
}

__device__ __forceinline__ FrameDev makeFrameD(Vec3 pmin, Vec3 pmax, float rot)
{
    FrameDev f;
    f.toFrame = qinv(angleAxis(rot, kUp));
    f.pMin = rotateVec(f.toFrame, pmin);
    f.pMax = rotateVec(f.toFrame, pmax);
    return f;
}

// PathfindToPoint (sim.cpp:5012-5035); goal_tri = NearestNavTri(pos)
__device__ Vec3 pathfindToPointD(const SceneDev &sc, Vec3 start, Vec3 pos, int goal_tri)
{
    const int start_tri = nearestNavTriD(sc, start);
    if (start_tri < 0 || goal_tri < 0) return v3(0.f, 0.f, 0.f); // (asserted in the reference)
    const int next = sc.astar[start_tri * sc.numNavTris + goal_tri];
    if (next == -1) return v3(0.f, 0.f, 0.f);
    if (next == goal_tri) return pos;
    return navTriCenterD(sc, next);
}

} // namespace mpenv
