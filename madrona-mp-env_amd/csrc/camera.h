// camera.h — what camera.hip (k_camera) and camera.cpp (the mpenv_camera_*
// entry points) share: the kernel's view of an enabled camera and its launcher.
#pragma once

#include <hip/hip_runtime.h>

#include "engine.h"

namespace mpenv {

// One allocation behind all three pointers: depth [A][height][width] f32, then
// label [A][height][width] u8, then the two ray tables (camera_core.h) as
// sx[128], sy[128] f32.
struct CameraDev {
    float *depth;
    uint8_t *label;
    const float *tab;
    int32_t width, height;
    int32_t tasksPerAgent; // width * height / 64: a wave task is 64 consecutive pixels of one agent's image
    int32_t pad;
};

// k_camera over the whole batch of `s` from its current state, on `stream`
int launchCamera(const DevState &s, const SceneDev &sc, const SceneImages &img, const CameraDev &cam, void *stream);

} // namespace mpenv
