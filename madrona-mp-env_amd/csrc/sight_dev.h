// sight_dev.h — the view tests of one (viewer, target) pair: k_vis's frustum
// test and the lane-wise isAgentVisible of k_sim's flank reward.
#pragma once
#include "sim_dev.h"

namespace mpenv {

// utils.cpp:169-184 inFrustum
__device__ __forceinline__ bool inFrustumD(const SceneDev &sc, Vec3 vp)
{
    bool in = true;
    in = in && vp.y * sc.frustum[1] - fabs_(vp.x) * sc.frustum[0] > -c::kAgentRadius;
    in = in && vp.y * sc.frustum[3] - fabs_(vp.z) * sc.frustum[2] > -c::kAgentRadius;
    return in;
}

__device__ __forceinline__ Vec3 visSamplePointD(const DevState &S, int64_t gt, Vec3 delta_right, int p)
{
    Vec3 pt = ldPos(S, gt);
    pt.z += p == 0 ? c::kAgentRadius : viewHeightD(S.curPose[gt]);
    if (p == 2) pt = pt - delta_right;
    if (p == 3) pt = pt + delta_right;
    return pt;
}

// utils.cpp:169-271 isAgentVisible for one (viewer, target) pair, lane-wise
// (the flank reward's checks; k_vis batches the opponent checks instead).
template <class LBVH>
__device__ __forceinline__ bool isAgentVisibleD(const DevState &S, const SceneDev &sc, const LBVH &bvh, int w, Vec3 org,
                                Quat aim_rot, int target)
{
    const int N = S.N;
    const int64_t g0 = (int64_t)w * N;
    const Quat inv_rot = qinv(aim_rot);
    const Vec3 delta_right = rotateVec(aim_rot, kRight) * 0.9f * c::kAgentRadius;
    for (int p = 0; p < 4; p++) {
        Vec3 to_test = visSamplePointD(S, g0 + target, delta_right, p) - org;
        Vec3 view = rotateVec(inv_rot, to_test);
        if (view.y <= 0.f) continue;
        if (!inFrustumD(sc, view)) continue;
        const float len = length(to_test);
        if (len < c::kAgentRadius) continue;
        to_test = to_test / len;
        if (visibleRayD(bvh, S.px, S.py, S.pz, g0, N, org, to_test, target)) return true;
    }
    return false;
}

} // namespace mpenv
