// camera_core.h — the egocentric depth camera's model (DESIGN.md §2
// definition 18): one definition for the host (mpenv_camera_rays, the test
// expectation) and the device (k_camera), compiled on both sides with
// -ffp-contract=off like mpenv_core.h, whose rotateVec and normalize are all
// the arithmetic it does.
//
// A camera is width x height pixels (multiples of 8 in [8, 128]) with a
// horizontal field of view hfov_deg in (0, 170).  Pixel (r, c), row 0 at the
// top, looks through the image plane at distance 1 in front of the eye at
//   sx[c] = tan(hfov/2) * ((2c + 1) / width - 1)
//   sy[r] = tan(hfov/2) * (height / width) * (1 - (2r + 1) / height)
// (square pixels).  The two tables are evaluated once on the host in double
// precision and rounded to float; the device reads them and evaluates no
// tangent.  The ray of an agent starts at pos + (0, 0, viewHeight(curPose)),
// on its own capsule's axis where its eyes are for sight and shots, and runs
// along normalize((fwd + sx[c] * right) + sy[r] * up) of its aim quaternion.
#pragma once

#include <math.h>

#include "mpenv_core.h"

namespace mp {

constexpr int kCameraMinDim = 8, kCameraMaxDim = 128;
constexpr float kCameraMaxFov = 170.f;

// viewHeight: consts.hpp's standHeight, crouchHeight and proneHeight (65, 47,
// 30) less agentRadius (15), the kernels' viewHeightD; camera.hip asserts that
// the two agree
MP_HD constexpr float cameraViewHeight(int pose) { return pose == 0 ? 50.f : (pose == 1 ? 32.f : 15.f); }

// null when the configuration is one a camera can have, else what is wrong with it
inline const char *cameraConfigError(int width, int height, float hfov_deg)
{
    if (width < kCameraMinDim || width > kCameraMaxDim || width % 8 != 0)
        return "camera width must be a multiple of 8 in [8, 128]";
    if (height < kCameraMinDim || height > kCameraMaxDim || height % 8 != 0)
        return "camera height must be a multiple of 8 in [8, 128]";
    if (!(hfov_deg > 0.f && hfov_deg < kCameraMaxFov)) return "camera hfov_deg must be in (0, 170)";
    return nullptr;
}

// sx[width], sy[height]; host only (double precision, rounded once)
inline void cameraTables(int width, int height, float hfov_deg, float *sx, float *sy)
{
    const double th = tan(0.5 * (double)hfov_deg * 3.14159265358979323846 / 180.0);
    for (int c = 0; c < width; c++) sx[c] = (float)(th * ((double)(2 * c + 1) / (double)width - 1.0));
    for (int r = 0; r < height; r++)
        sy[r] = (float)(th * ((double)height / (double)width) * (1.0 - (double)(2 * r + 1) / (double)height));
}

MP_HD Vec3 cameraOrigin(Vec3 pos, int pose)
{
    pos.z += cameraViewHeight(pose);
    return pos;
}

MP_HD Vec3 cameraRayDir(Quat aim, float sx, float sy)
{
    const Vec3 fwd = rotateVec(aim, kFwd), right = rotateVec(aim, kRight), up = rotateVec(aim, kUp);
    return normalize((fwd + sx * right) + sy * up);
}

} // namespace mp
