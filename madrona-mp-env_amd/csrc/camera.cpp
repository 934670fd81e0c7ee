// camera.cpp — the egocentric depth camera's entry points
// (include/mpenv_camera.h): configuration, the two image buffers, the render
// behind every step, and the host restatement of the rays (camera_core.h).
#include <cstring>

#include "manager.h"

#include "camera_core.h"

namespace {

int badConfig(const mpenv_camera_config *cfg)
{
    if (!cfg) return fail(MPENV_ERR_INVALID, "null argument");
    if (const char *why = mp::cameraConfigError(cfg->width, cfg->height, cfg->hfov_deg)) return fail(MPENV_ERR_INVALID, why);
    return MPENV_OK;
}

int disabled(const char *who)
{
    return fail(MPENV_ERR_INVALID, std::string(who) + ": the camera is disabled (mpenv_camera_enable first)");
}

constexpr size_t kTabBytes = 2 * mp::kCameraMaxDim * sizeof(float);

} // namespace

void mpenv_manager::renderCamera(hipStream_t st)
{
    // each range against its own scene, into its agents' images
    for (const MapRange &r : ranges) {
        CameraDev rc = cam;
        const int64_t px = (int64_t)r.w0 * S.N * cam.height * cam.width;
        rc.depth += px;
        rc.label += px;
        launched(launchCamera(r.S, r.sc, scenes[r.scene].img, rc, st), "k_camera launch failed");
    }
}

extern "C" {

int mpenv_camera_layout(const mpenv_camera_config *cfg, uint32_t num_worlds, uint32_t team_size, int64_t *depth_bytes,
                        int64_t *label_bytes)
{
    if (int rc = badConfig(cfg)) return rc;
    if (num_worlds == 0 || team_size == 0 || team_size > (uint32_t)kMaxTeamSize)
        return fail(MPENV_ERR_INVALID, "num_worlds must be >= 1 and team_size in [1, 6]");
    const int64_t px = (int64_t)num_worlds * 2 * team_size * cfg->height * cfg->width;
    if (depth_bytes) *depth_bytes = px * 4;
    if (label_bytes) *label_bytes = px;
    return MPENV_OK;
}

int mpenv_camera_rays(const mpenv_camera_config *cfg, int32_t n, const float *pos, const float *aim_quat,
                      const int32_t *cur_pose, float *org_out, float *dir_out)
{
    if (int rc = badConfig(cfg)) return rc;
    if (n < 0 || !pos || !aim_quat || !cur_pose || !org_out || !dir_out) return fail(MPENV_ERR_INVALID, "bad argument");
    float sx[mp::kCameraMaxDim], sy[mp::kCameraMaxDim];
    mp::cameraTables(cfg->width, cfg->height, cfg->hfov_deg, sx, sy);
    for (int32_t k = 0; k < n; k++) {
        const mp::Vec3 o = mp::cameraOrigin(mp::v3(pos[3 * k], pos[3 * k + 1], pos[3 * k + 2]), cur_pose[k]);
        org_out[3 * k] = o.x;
        org_out[3 * k + 1] = o.y;
        org_out[3 * k + 2] = o.z;
        const mp::Quat q = mp::quat(aim_quat[4 * k], aim_quat[4 * k + 1], aim_quat[4 * k + 2], aim_quat[4 * k + 3]);
        float *d = dir_out + (size_t)k * cfg->height * cfg->width * 3;
        for (int r = 0; r < cfg->height; r++)
            for (int c = 0; c < cfg->width; c++, d += 3) {
                const mp::Vec3 v = mp::cameraRayDir(q, sx[c], sy[r]);
                d[0] = v.x;
                d[1] = v.y;
                d[2] = v.z;
            }
    }
    return MPENV_OK;
}

int mpenv_camera_enable(mpenv_manager *m, const mpenv_camera_config *cfg)
{
    if (!m) return fail(MPENV_ERR_INVALID, "null manager");
    if (int rc = badConfig(cfg)) return rc;
    const int64_t px = m->S.A * cfg->height * cfg->width;
    if (px / 64 >= (int64_t)1 << 31) return fail(MPENV_ERR_INVALID, "camera too large for this batch (2^31 wave tasks)");
    return guarded([&] {
        // the new camera is built aside and swapped in whole: a failed
        // allocation leaves the previous one, or none, in place
        DevPtr buf;
        try {
            buf = DevPtr::create((size_t)px * 5 + kTabBytes);
        } catch (...) {
            (void)hipGetLastError(); // the next launch's error check must not see this one
            throw;
        }
        char *base = static_cast<char *>(buf.get());
        float tab[2 * mp::kCameraMaxDim] = {};
        mp::cameraTables(cfg->width, cfg->height, cfg->hfov_deg, tab, tab + mp::kCameraMaxDim);
        HIP_CHECK(hipMemsetAsync(base, 0, (size_t)px * 5, m->stream));
        m->upload(base + px * 5, tab, kTabBytes); // waits for the stream: no render of the old camera is in flight on it
        CameraDev cam {};
        cam.depth = reinterpret_cast<float *>(base);
        cam.label = reinterpret_cast<uint8_t *>(base + px * 4);
        cam.tab = reinterpret_cast<const float *>(base + px * 5);
        cam.width = cfg->width;
        cam.height = cfg->height;
        cam.tasksPerAgent = cfg->width * cfg->height / 64;
        m->cam = cam;
        m->camCfg = *cfg;
        m->camCfg.reserved = 0;
        m->camBuf = std::move(buf); // the previous buffer goes with `buf`
        m->camOn = true;
    });
}

int mpenv_camera_disable(mpenv_manager *m)
{
    if (!m) return fail(MPENV_ERR_INVALID, "null manager");
    return guarded([&] {
        HIP_CHECK(hipStreamSynchronize(m->stream));
        m->camOn = false;
        m->cam = CameraDev {};
        m->camBuf = DevPtr {};
    });
}

int mpenv_camera_enabled(mpenv_manager *m, mpenv_camera_config *out, int32_t *on)
{
    if (!m || !on) return fail(MPENV_ERR_INVALID, "null argument");
    *on = m->camOn ? 1 : 0;
    if (out) *out = m->camOn ? m->camCfg : mpenv_camera_config {};
    return MPENV_OK;
}

int mpenv_camera_render(mpenv_manager *m, void *stream)
{
    if (!m) return fail(MPENV_ERR_INVALID, "null manager");
    if (!m->camOn) return disabled("mpenv_camera_render");
    return guarded([&] {
        m->renderCamera(streamOf(m, stream));
        if (!stream) HIP_CHECK(hipStreamSynchronize(m->stream));
    });
}

int mpenv_camera_tensor(mpenv_manager *m, int32_t which, void **ptr, int32_t *dtype, int32_t *ndim, int64_t *dims,
                        int32_t *gpu_id)
{
    if (!m || !ptr || !dtype || !ndim || !dims) return fail(MPENV_ERR_INVALID, "null argument");
    if (!m->camOn) return disabled("mpenv_camera_tensor");
    if (which != MPENV_CAMERA_DEPTH && which != MPENV_CAMERA_LABEL)
        return fail(MPENV_ERR_INVALID, "camera tensor must be MPENV_CAMERA_DEPTH or MPENV_CAMERA_LABEL");
    *ptr = which == MPENV_CAMERA_DEPTH ? (void *)m->cam.depth : (void *)m->cam.label;
    *dtype = which == MPENV_CAMERA_DEPTH ? MPENV_DTYPE_FLOAT32 : MPENV_DTYPE_UINT8;
    *ndim = 3;
    dims[0] = m->S.A;
    dims[1] = m->cam.height;
    dims[2] = m->cam.width;
    if (gpu_id) *gpu_id = m->gpu;
    return MPENV_OK;
}

} // extern "C"
