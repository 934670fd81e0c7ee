"""The one ctypes binding of the engine's C ABI (include/mpenv.h): the
structures it takes and SIGNATURES, {function: (restype, [argtypes])}, for
every function the header declares.  bind(lib) installs the table on a CDLL
handle; tests/test_abi.py::test_binding_table_matches_header pins it to the
header.  Imports nothing but ctypes.

One type per parameter kind: c_void_p for the manager handle, streams, device
pointers and host buffers that callers hand over as plain addresses
(arr.ctypes.data); POINTER(c_xxx) for host out-parameters passed with byref;
c_char_p for host strings."""
import ctypes as C

vp, cstr = C.c_void_p, C.c_char_p
i32, u32, i64 = C.c_int32, C.c_uint32, C.c_int64
P = C.POINTER


class MpenvConfig(C.Structure):
    _fields_ = [
        ("exec_mode", C.c_int32), ("gpu_id", C.c_int32), ("num_worlds", C.c_uint32),
        ("rand_seed", C.c_uint32), ("auto_reset", C.c_int32), ("sim_flags", C.c_uint32),
        ("task_type", C.c_int32), ("team_size", C.c_uint32), ("num_pbt_policies", C.c_uint32),
        ("policy_history_size", C.c_uint32), ("scene_path", C.c_char_p), ("train_flank", C.c_int32),
        ("replay_log_path", C.c_char_p), ("record_log_path", C.c_char_p),
        ("event_log_path", C.c_char_p), ("curriculum_data_path", C.c_char_p),
        ("world_id_offset", C.c_uint32),
    ]


class XlaOpaque(C.Structure):
    _fields_ = [("magic", C.c_uint32), ("version", C.c_uint32), ("manager", C.c_uint64),
                ("num_buffers", C.c_int32), ("reserved", C.c_int32)]


class GeomQueries(C.Structure):
    _fields_ = [("o", C.c_void_p), ("d", C.c_void_p), ("caps", C.c_void_p), ("sel", C.c_void_p),
                ("bound", C.c_void_p), ("z1", C.c_void_p), ("hint", C.c_void_p), ("t", C.c_void_p),
                ("normal", C.c_void_p), ("i0", C.c_void_p), ("i1", C.c_void_p), ("num_caps", C.c_int32),
                ("sub", C.c_int32)]


_XLA = [vp, P(vp), cstr, C.c_size_t]  # stream, buffers, opaque, opaque_len
_BVH = [cstr, vp, P(i32), vp, P(i32), P(i32)]  # scene, nodes_out, num_nodes, verts_out, num_verts, max_stack

SIGNATURES = {
    "mpenv_create": (i32, [P(MpenvConfig), P(vp)]),
    "mpenv_destroy": (None, [vp]),
    "mpenv_init": (i32, [vp]),
    "mpenv_step": (i32, [vp]),
    "mpenv_step_async": (i32, [vp, vp]),
    "mpenv_gpu_stream_init": (i32, [vp, vp, P(vp)]),
    "mpenv_gpu_stream_step": (i32, [vp, vp, P(vp)]),
    "mpenv_xla_opaque_make": (i32, [vp, P(XlaOpaque)]),
    "mpenv_xla_gpu_stream_init": (None, _XLA),
    "mpenv_xla_gpu_stream_step": (None, _XLA),
    "mpenv_xla_gpu_stream_init_status": (None, _XLA + [vp]),
    "mpenv_xla_gpu_stream_step_status": (None, _XLA + [vp]),
    "mpenv_xla_errors": (i64, []),
    "mpenv_export_tensor": (i32, [vp, i32, P(vp), P(i32), P(i32), P(i64), P(i32)]),
    "mpenv_export_layout": (i32, [i32, u32, u32, P(i32), P(i32), P(i64)]),
    "mpenv_train_interface_size": (i32, [P(i32), P(i32)]),
    "mpenv_train_interface_entry": (i32, [i32, i32, P(cstr), P(i32)]),
    "mpenv_copy_actions": (i32, [vp, vp, vp]),
    "mpenv_combat_actions": (i32, [vp, vp, vp, i32, vp]),
    "mpenv_debug_trace_rays": (i32, [vp, vp, vp, i32, i32, vp, vp, vp]),
    "mpenv_debug_geom_queries": (i32, [vp, i32, i32, P(GeomQueries), vp]),
    "mpenv_wire_bytes": (i32, [vp, i32, P(i64)]),
    "mpenv_wire_pack": (i32, [vp, vp, i32, vp]),
    "mpenv_wire_unpack": (i32, [vp, vp, i32, vp]),
    "mpenv_wire_error": (i32, [vp, P(u32)]),
    "mpenv_wire_error_async": (i32, [vp, vp, vp]),  # out: pinned host memory, by address
    "mpenv_state_bytes": (i32, [vp, P(i64)]),
    "mpenv_state_save": (i32, [vp, vp, vp]),
    "mpenv_state_load": (i32, [vp, vp, vp, vp]),
    "mpenv_state_error": (i32, [vp, P(u32)]),
    "mpenv_state_dims": (i32, [vp, P(u32), P(u32), P(u32)]),
    "mpenv_state_section": (i32, [i32, u32, u32, u32, P(cstr), P(i64), P(i64), P(i32), P(i32), P(i32)]),
    "mpenv_state_section_dtype": (i32, [i32, P(i32)]),
    "mpenv_policy_check": (i32, [cstr]),
    "mpenv_policy_load": (i32, [vp, cstr]),
    "mpenv_policy_unload": (i32, [vp]),
    "mpenv_policy_loaded": (i32, [vp, P(i32)]),
    "mpenv_policy_forward": (i32, [vp, vp, vp, vp]),
    "mpenv_debug_policy_step": (i32, [vp, i32, vp]),
    "mpenv_debug_policy_dense": (i32, [vp, vp, i32, i32, vp, i32, vp, vp]),
    "mpenv_graph_captures": (i32, [vp, P(i64)]),
    "mpenv_graph_status": (i32, [vp, P(i32), cstr, i32]),
    "mpenv_set_world_groups": (i32, [vp, i32]),
    "mpenv_world_groups": (i32, [vp, P(i32)]),
    "mpenv_set_lidar_branch": (i32, [vp, i32]),
    "mpenv_set_lidar_iters": (i32, [vp, i32]),
    "mpenv_trigger_reset": (i32, [vp, i32]),
    "mpenv_set_pvp_action": (i32, [vp, i32, i32, P(i32), P(C.c_float), P(i32)]),
    "mpenv_set_hp": (i32, [vp, i32, i32, i32]),
    "mpenv_set_agent_policy": (i32, [vp, i32, i32, i32]),
    "mpenv_set_uniform_agent_policy": (i32, [vp, i32]),
    "mpenv_is_replay_finished": (i32, [vp, P(i32)]),
    "mpenv_dims": (i32, [vp, P(i32), P(i32)]),
    "mpenv_kernel_timings": (i32, [vp, i32, P(cstr), P(C.c_float), P(i32)]),
    "mpenv_enable_kernel_timing": (i32, [vp, i32]),
    "mpenv_enable_stats": (i32, [vp, i32]),
    "mpenv_read_stats": (i32, [vp, vp, i32]),
    "mpenv_scene_bvh": (i32, _BVH),
    "mpenv_scene_lidar_bvh": (i32, _BVH),
    "mpenv_scene_bvh_variant": (i32, [cstr, vp, i32] + _BVH[1:]),
    "mpenv_scene_quirk_grid": (i32, [cstr, vp, vp, P(i32)]),
    "mpenv_scene_navmesh": (i32, [cstr, vp, P(i32), vp, vp]),
    "mpenv_last_error": (cstr, []),
    "mpenv_abi_version": (i32, []),
}


def bind(lib):
    """Install every signature on a CDLL handle of the library; returns it."""
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib
