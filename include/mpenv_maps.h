/* mpenv_maps.h -- map sets: one batch over several maps, a world range per
 * map (DESIGN.md §2 definition 19, INTEGRATION.md "Several maps in one
 * batch").  Included by mpenv.h; callers include that.
 *
 * A map set is an ordered list of ranges (scene directory, number of worlds).
 * Range r covers worlds [w0_r, w0_r + n_r), w0_r the sum of the counts in
 * front of it, and the counts sum to cfg->num_worlds.  Every world of range r
 * computes, bit for bit, what it would compute in a manager made by
 * mpenv_create on that directory with the same seed, flags, task and team
 * size and the same global world id (world_id_offset + w0_r + its index in
 * the range).  Worlds never read each other, so a step is the five step
 * kernels launched once per range, in range order on the step's stream, each
 * launch with that range's slice of the state and its scene; the captured
 * step graph holds all of them.  Equal paths are loaded and uploaded once and
 * share one scene index; the ranges themselves are never merged.
 *
 * mpenv_create_maps refuses, with MPENV_ERR_INVALID and a message that names
 * the range index and its directory: cfg->scene_path set as well, n outside
 * [1, MPENV_MAX_MAP_RANGES], a range without worlds, counts that do not sum
 * to cfg->num_worlds, a map neither residency supports
 * (mpenv_scene_residency.h), and a map the task or the flags rule out
 * (ZoneCaptureDefend needs 4 zones, SubZones 3, SpawnInMiddle free middle
 * cells).  A directory that does not load is MPENV_ERR_IO.
 * replay_log_path, record_log_path, event_log_path and curriculum_data_path
 * are MPENV_ERR_UNSUPPORTED: snapshot positions belong to one map.  All of
 * this is decided before the GPU is touched, by the code mpenv_maps_plan runs.
 *
 * On a map-set manager every call of mpenv.h works as on any other, except:
 *   mpenv_set_world_groups(n > 1), mpenv_set_lidar_branch(1) and
 *   mpenv_wire_bytes / _pack / _unpack   MPENV_ERR_UNSUPPORTED (the ranges
 *       are the groups and run in order on one stream; the wire message is
 *       one view over the batch and its observation kernel takes one scene);
 *       MPENV_WORLD_GROUPS and MPENV_LIDAR_BRANCH are ignored;
 *   mpenv_scene_residency                MPENV_ERR_INVALID: one answer would
 *       be wrong for a mixed set; mpenv_map_info reports each range's;
 *   mpenv_set_scene_residency            applies to every scene: AUTO
 *       resolves per scene, LDS is refused (naming the map, nothing changed)
 *       when any scene does not fit;
 *   mpenv_debug_trace_rays, mpenv_debug_geom_queries   answer for range 0's
 *       scene;
 *   mpenv_state_load                     a world map that takes a world's
 *       state from a snapshot world of another scene raises
 *       MPENV_STATE_ERR_CROSS_MAP and the load writes nothing; forks between
 *       ranges that share a scene are fine.  A snapshot of another range
 *       layout (counts, or a scene's collisions.bin) is MPENV_STATE_ERR_HEADER.
 *   mpenv_state_dims                     spawn_track_len is the largest of
 *       the scenes' (the row shape every range shares).
 *
 * mpenv_maps_plan needs no GPU and no manager: `out` (n entries) receives
 * what mpenv_create_maps would make of the list, range by range, with
 * `residency` what MPENV_SCENE_AUTO picks; a map refused on its own has
 * supported = 0 and the reason, and the call returns the code and message
 * mpenv_create_maps would. */
#ifndef MPENV_MAPS_H
#define MPENV_MAPS_H

#include "mpenv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPENV_MAX_MAP_RANGES 32
#define MPENV_STATE_ERR_CROSS_MAP 4u

typedef struct mpenv_map_range {
    const char *scene_path;
    uint32_t num_worlds;
} mpenv_map_range;

typedef struct mpenv_map_desc {            /* one range, as the engine holds it */
    int32_t first_world, num_worlds;
    int32_t scene;                         /* index of the loaded scene; equal paths share one */
    int32_t residency;                     /* MPENV_SCENE_LDS / _GLOBAL in use (plan: what AUTO picks) */
    int32_t supported;                     /* plan only */
    char reason[128];                      /* plan only */
} mpenv_map_desc;

/* cfg->scene_path must be null; cfg->num_worlds must equal the sum */
int mpenv_create_maps(const mpenv_config *cfg, const mpenv_map_range *maps, int32_t n, mpenv_manager **out);
int mpenv_num_maps(mpenv_manager *mgr, int32_t *n);            /* 1 for a manager from mpenv_create */
int mpenv_map_info(mpenv_manager *mgr, int32_t range, mpenv_map_desc *out, const char **scene_path);
/* int32 [W] on the device: range index per world.  Read-only: the engine's own table, which
 * mpenv_state_load's check reads (an entry written from outside cannot index past the ranges, but it
 * makes the cross-map check answer for the wrong range) */
int mpenv_map_of_world(mpenv_manager *mgr, void **dev_ptr);
/* no GPU, no manager: what mpenv_create_maps would make of the list, range by range */
int mpenv_maps_plan(const mpenv_config *cfg, const mpenv_map_range *maps, int32_t n,
                    mpenv_map_desc *out, int32_t *spawn_track_len);

#ifdef __cplusplus
}
#endif

#endif /* MPENV_MAPS_H */
