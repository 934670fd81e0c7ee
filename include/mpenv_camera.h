/* mpenv_camera.h -- the egocentric depth camera (DESIGN.md §2 definition 18,
 * INTEGRATION.md "Camera observations").  Included by mpenv.h; callers include
 * that.  An extension: the reference renders only in its viewer.
 *
 * While a camera is enabled every agent has two images of what it looks at,
 * [A][height][width] in agent order (world-major, as every per-agent export):
 *   MPENV_CAMERA_DEPTH  f32  distance along the pixel's ray to the closest hit
 *                            of traceRayAgainstWorld, at most the scene's
 *                            lidar range (the value a lidar ray reports), -1
 *                            where the ray hits nothing;
 *   MPENV_CAMERA_LABEL  u8   0 nothing, 1 map geometry, 2 a teammate's
 *                            capsule, 3 an opponent's.
 * The pinhole model: width and height are multiples of 8 in [8, 128],
 * hfov_deg is the horizontal field of view in (0, 170), pixels are square.
 * Pixel (r, c), row 0 at the top, looks along
 *   normalize(fwd + sx[c] * right + sy[r] * up)   of the agent's aim rotation,
 *   sx[c] = tan(hfov / 2) * ((2c + 1) / width - 1),
 *   sy[r] = tan(hfov / 2) * (height / width) * (1 - (2r + 1) / height),
 * from the agent's position raised by its pose's view height (stand 50,
 * crouch 32, prone 15).  The map is the lidar's tree; dead agents see and are
 * seen as live ones, as with the lidar.
 *
 * When the images are written: while enabled, behind the kernels of every
 * step and every init -- mpenv_step, mpenv_step_async, mpenv_gpu_stream_step,
 * mpenv_init, mpenv_gpu_stream_init -- on that call's stream, and by
 * mpenv_camera_render from the current state without a step (hip_stream null:
 * the manager's own stream, and the call waits for it).  The step itself is
 * unchanged: the same captured graph with the camera on or off.  After
 * mpenv_camera_enable the images are zeros until the first of these.
 *
 * The images are no part of the state: not in snapshots, not on the wire, not
 * in the trainInterface, and no export id names them.  After mpenv_state_load
 * they are still those of the last render, until the next step or
 * mpenv_camera_render.
 *
 * mpenv_camera_enable allocates A * height * width * 5 bytes; called again
 * with another configuration it replaces the camera (call it between steps).
 * A configuration outside the limits above is MPENV_ERR_INVALID with the limit
 * named; an allocation that fails is MPENV_ERR_HIP and leaves the previous
 * camera, or none, in place.  mpenv_camera_tensor and mpenv_camera_render
 * while disabled are MPENV_ERR_INVALID.  The pointers mpenv_camera_tensor
 * returns hold until the next enable or disable.
 *
 * Without a manager or a GPU: mpenv_camera_layout gives the two buffers'
 * bytes for a batch, and mpenv_camera_rays the model itself -- for n agents'
 * positions, aim quaternions (w, x, y, z) and poses (0 stand, 1 crouch, 2
 * prone) the ray origins [n][3] and directions [n][height][width][3], bit for
 * bit what the kernel traces. */
#ifndef MPENV_CAMERA_H
#define MPENV_CAMERA_H

#include "mpenv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPENV_CAMERA_DEPTH 0
#define MPENV_CAMERA_LABEL 1

typedef struct mpenv_camera_config {
    int32_t width, height;
    float hfov_deg;
    int32_t reserved;
} mpenv_camera_config;

int mpenv_camera_enable(mpenv_manager *mgr, const mpenv_camera_config *cfg);
int mpenv_camera_disable(mpenv_manager *mgr);
int mpenv_camera_enabled(mpenv_manager *mgr, mpenv_camera_config *out /* may be null */, int32_t *on);
int mpenv_camera_render(mpenv_manager *mgr, void *hip_stream);
int mpenv_camera_tensor(mpenv_manager *mgr, int32_t which, void **ptr, int32_t *dtype, int32_t *ndim, int64_t *dims,
                        int32_t *gpu_id);
int mpenv_camera_layout(const mpenv_camera_config *cfg, uint32_t num_worlds, uint32_t team_size, int64_t *depth_bytes,
                        int64_t *label_bytes);
int mpenv_camera_rays(const mpenv_camera_config *cfg, int32_t n, const float *pos, const float *aim_quat,
                      const int32_t *cur_pose, float *org_out, float *dir_out);

#ifdef __cplusplus
}
#endif

#endif /* MPENV_CAMERA_H */
