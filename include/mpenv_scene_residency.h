/* mpenv_scene_residency.h -- where a scene's BVH images live while the step
 * kernels walk them, and what a scene directory asks of the engine (DESIGN.md
 * §3 "Scene residency", INTEGRATION.md "Bringing your own map").  Included by
 * mpenv.h; callers include that.
 *
 * k_move, k_sim, k_vis and k_lidar (and the ray / geometry test hooks) read
 * the collision tree, its sphere-cast image and the lidar tree's eight octant
 * images either
 *   MPENV_SCENE_LDS     from a copy each block stages into its LDS.  The
 *                       scene must have at most 256 nodes per tree and stack
 *                       bounds of at most 16 (the traversal keeps byte-sized
 *                       node indices in registers), and every kernel's
 *                       dynamic LDS request must fit 64 KB; or
 *   MPENV_SCENE_GLOBAL  from images built once at mpenv_create in global
 *                       memory (they stay in the L2 cache).  Stack bounds up
 *                       to 64, any node count.
 * Both compute the same values bit for bit: the traversal is one source
 * compiled twice.  MPENV_SCENE_AUTO picks LDS whenever the scene meets its
 * limits and GLOBAL otherwise; that is the default, which the environment
 * variable MPENV_SCENE_RESIDENCY=auto|lds|global replaces at mpenv_create.
 *
 * mpenv_set_scene_residency may be called at any time between steps; the
 * captured step graph is re-captured by the next step when the path in use
 * changed.  MPENV_SCENE_LDS on a scene that does not fit, or any other value,
 * is MPENV_ERR_INVALID (mpenv_last_error names the limit) and changes nothing.
 * mpenv_scene_residency reports the path in use, MPENV_SCENE_LDS or
 * MPENV_SCENE_GLOBAL, never AUTO.
 *
 * A scene neither path supports is refused by mpenv_create with the reason
 * named: a stack bound above 64, more than 65,534 collision triangles
 * (k_vis's occluder hints are 16-bit triangle indices), or spawn lists that
 * do not fit k_sim's LDS.
 *
 * mpenv_scene_info loads a scene directory and reports all of this without a
 * GPU or a manager.  lds_bytes_* are the dynamic LDS bytes each kernel would
 * ask for on the LDS path (k_vis's for the team size that needs the most);
 * `residency` is what AUTO would choose; supported = 0 comes with the reason
 * in `reason` (and residency = MPENV_SCENE_AUTO); return value MPENV_ERR_IO
 * when the directory cannot be loaded. */
#ifndef MPENV_SCENE_RESIDENCY_H
#define MPENV_SCENE_RESIDENCY_H

#include "mpenv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPENV_SCENE_AUTO 0
#define MPENV_SCENE_LDS 1
#define MPENV_SCENE_GLOBAL 2

typedef struct mpenv_scene_info_t {
    int32_t triangles;                          /* of the collision tree */
    int32_t collision_nodes, collision_stack;   /* stack: the larger of the reference-order and any-order bounds */
    int32_t lidar_nodes, lidar_stack;
    int32_t lidar_triangles;
    int32_t residency;                          /* what MPENV_SCENE_AUTO chooses */
    int32_t supported;
    int64_t lds_bytes_move, lds_bytes_sim, lds_bytes_vis, lds_bytes_lidar;
    int64_t global_bytes;                       /* of the global-resident images */
    char reason[128];
} mpenv_scene_info_t;

int mpenv_set_scene_residency(mpenv_manager *mgr, int32_t mode);
int mpenv_scene_residency(mpenv_manager *mgr, int32_t *mode_in_use);
int mpenv_scene_info(const char *scene_path, mpenv_scene_info_t *out);

#ifdef __cplusplus
}
#endif

#endif /* MPENV_SCENE_RESIDENCY_H */
