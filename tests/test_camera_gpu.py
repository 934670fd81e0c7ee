"""k_camera on the device (csrc/camera.hip, include/mpenv_camera.h; DESIGN.md §2
definition 18) against the expectation camera_testlib builds from the oracle's
parts, bit for bit: the depth by its bit patterns, the label by value.

The shapes are the smallest at which the kernel can go wrong: 1 world 1v1
(2 agents: fewer capsules than the cull's lanes, one nearly empty block), 3
worlds 3v3 (18 agents) and 5 worlds 6v6 (60 agents: a block's partial range);
8 x 8 (one wave task per agent), 16 x 8, 24 x 16 (a width that is no power of
two: tasks that straddle rows) and, once, 64 x 32 (a row per task, 32 tasks per
agent).  tests/test_camera_rays.py checks on the CPU that every configuration
holds every label and a clamped pixel."""
import numpy as np
import pytest

import camera_testlib as K
import mpenv_testlib as T
import scene_residency_testlib as R

pytestmark = pytest.mark.gpu


def engine(name, residency=None, groups=None, camera=True):
    c = K.CONFIGS[name]
    e = T.Engine(c["W"], c["team"], scene=K.scene_of(name))
    e.put_ctrl([0, 1, 1])
    if residency is not None:
        assert R.set_residency(e, residency) == 0, e.lib.mpenv_last_error().decode()
    if groups is not None:
        e.set_world_groups(groups)
    if camera:
        assert K.enable(e, K.config(*c["cam"])) == 0, e.lib.mpenv_last_error().decode()
    return e


def run_rollout(e, name, after=None):
    """init and the plan's tape; the image after init and after each chosen step is the builder's."""
    cfg, tape, steps, posed = K.plan(name)
    want = dict(steps)
    e.init()
    if -1 in want:
        K.check_images(e, want[-1], f"{name} after init")
    for s, acts in enumerate(tape):
        e.set_actions(acts)
        e.step()
        if s in want:
            K.check_images(e, want[s], f"{name} after step {s}")
            if after:
                after(s)


def sections(e):
    w, t, l = T.state_dims(e)
    out, k = {}, 0
    while True:
        sec = T.state_section(k, w, t, l)
        if sec is None:
            return out
        out[sec["name"]] = sec
        k += 1


def load_posed(e, blob, pos, quat, pose):
    """Overwrites positions, aim quaternions and poses in the snapshot at `blob` through the offsets
    mpenv_state_section names, and loads it."""
    sec = sections(e)
    cols = dict(px=pos[:, 0], py=pos[:, 1], pz=pos[:, 2], aw=quat[:, 0], ax=quat[:, 1], ay=quat[:, 2], az=quat[:, 3])
    for nm, col in cols.items():
        col = np.ascontiguousarray(col, np.float32)
        assert sec[nm]["bytes"] == col.nbytes
        e.mem.h2d(blob + sec[nm]["offset"], col)
    col = np.ascontiguousarray(pose, np.int32)
    assert sec["curPose"]["bytes"] == col.nbytes
    e.mem.h2d(blob + sec["curPose"]["offset"], col)
    e.state_load(blob)
    assert e.state_error() == 0


def run_posed(e, name):
    """The chosen poses: each loaded from an edited snapshot and rendered without a step.  The image
    is re-rendered, not restored: straight after the load it is still the previous one."""
    cfg, tape, steps, posed = K.plan(name)
    blob = e.new_state_blob()
    e.state_save(blob)
    prev = K.images(e)
    for nm, pos, quat, pose, exp in posed:
        load_posed(e, blob, pos, quat, pose)
        e.mem.hip.hipDeviceSynchronize()
        now = K.images(e)
        T.compare(now[0], prev[0], f"{name} {nm}: depth after the load, before a render")
        T.compare(now[1], prev[1], f"{name} {nm}: label after the load, before a render")
        assert K.render(e) == 0, e.lib.mpenv_last_error().decode()
        K.check_images(e, exp, f"{name} posed {nm}")
        prev = exp
    e.mem.free(blob)


@pytest.mark.parametrize("name", ["1x1v1_8x8", "3x3v3_16x8", "5x6v6_24x16", "5x6v6_64x32"])
def test_images_match_the_expectation(name):
    e = engine(name)
    assert R.residency(e) == R.LDS
    run_rollout(e, name)
    run_posed(e, name)
    e.close()


def test_global_residency_gives_the_same_images():
    """simple_map walked from the global-resident images: the expectation the LDS path met."""
    name = "3x3v3_16x8"
    e = engine(name, residency=R.GLOBAL)
    assert R.residency(e) == R.GLOBAL
    run_rollout(e, name)
    run_posed(e, name)
    # and back, between two renders of one state
    glob = K.images(e)
    assert R.set_residency(e, R.LDS) == 0 and K.render(e) == 0
    lds = K.images(e)
    T.compare(lds[0], glob[0], "depth: LDS against global")
    T.compare(lds[1], glob[1], "label: LDS against global")
    e.close()


def test_a_scene_beyond_lds_renders_from_global_memory():
    name = "pillars_3x3v3_16x8"
    rc, info = R.scene_info(K.scene_of(name))
    assert rc == 0 and info.lidar_nodes > 256
    e = engine(name)
    assert R.residency(e) == R.GLOBAL  # what "auto" chose
    run_rollout(e, name)
    run_posed(e, name)
    e.close()


def test_world_groups_give_equal_images():
    name = "5x6v6_24x16"
    for groups in (1, 3):
        e = engine(name, groups=groups)
        run_rollout(e, name)
        e.close()


def test_render_is_pure_and_the_step_is_untouched():
    """render_camera after a step reproduces the in-step image, twice over; and 30 steps with the
    camera on leave the shipped trainInterface outputs (every one but the two agent maps, which no
    step writes), the debug state and the graph's capture count exactly those of an engine with it
    off."""
    name = "3x3v3_16x8"
    cfg, tape, steps, posed = K.plan(name)
    on, off = engine(name), engine(name, camera=False)
    on.init()
    off.init()
    for s in range(30):
        acts = T.seek_combat_actions(off, s)
        for e in (on, off):
            e.set_actions(acts)
            e.step()
        if s in (0, 7, 29):
            for n in list(T.TRAIN_OUTPUTS.values()) + T.DEBUG_OUTPUTS:
                T.compare(on.get(n), off.get(n), f"{n} @ step {s}: camera on against off")
    assert on.graph_captures() == off.graph_captures() >= 1
    in_step = K.images(on)
    exp = K.expected(cfg, *K.agent_state(on), 2 * K.CONFIGS[name]["team"])
    T.compare(in_step[0], exp[0], "in-step depth against the builder on the engine's own state")
    T.compare(in_step[1], exp[1], "in-step label")
    for k in range(2):
        assert K.render(on) == 0
        again = K.images(on)
        T.compare(again[0], in_step[0], f"depth after render {k}")
        T.compare(again[1], in_step[1], f"label after render {k}")
    for n in list(T.TRAIN_OUTPUTS.values()) + T.DEBUG_OUTPUTS:
        T.compare(on.get(n), off.get(n), f"{n} after the renders")
    # enabling and disabling never re-captures
    c0 = on.graph_captures()
    assert K.disable(on) == 0
    on.set_actions(tape[0])
    on.step()
    assert K.enable(on, cfg) == 0
    on.set_actions(tape[1])
    on.step()
    assert on.graph_captures() == c0
    on.close()
    off.close()


def test_lifecycle_and_errors():
    lib = K.lib()
    name = "1x1v1_8x8"
    e = engine(name, camera=False)
    e.init()
    assert K.enabled(e)[0] == 0
    rc = K.tensor(e, K.DEPTH)[0]
    assert rc == K.ERR_INVALID and "disabled" in lib.mpenv_last_error().decode()
    assert K.render(e) == K.ERR_INVALID and "disabled" in lib.mpenv_last_error().decode()
    for w, h, fov, needle in ((12, 8, 90.0, "width"), (8, 0, 90.0, "height"), (136, 8, 90.0, "width"),
                              (8, 8, 0.0, "hfov"), (8, 8, 170.0, "hfov")):
        assert K.enable(e, K.config(w, h, fov)) == K.ERR_INVALID and needle in lib.mpenv_last_error().decode()
        assert K.enabled(e)[0] == 0
    assert K.enable(e, K.config(8, 8, 60.0)) == 0
    on, cfg = K.enabled(e)
    assert (on, cfg.width, cfg.height, cfg.hfov_deg) == (1, 8, 8, 60.0)
    rc, p, dt, shape = K.tensor(e, K.LABEL)
    assert (rc, dt, shape) == (0, K.DTYPE_U8, (2, 8, 8)) and p
    assert K.tensor(e, 2)[0] == K.ERR_INVALID
    # zeros until the first render
    depth, label = K.images(e)
    assert not depth.any() and not label.any()
    state = K.agent_state(e)
    assert K.render(e) == 0
    K.check_images(e, K.expected(K.config(8, 8, 60.0), *state, 2), "first render after enable")
    # a refused re-enable leaves the camera as it is
    assert K.enable(e, K.config(8, 12, 60.0)) == K.ERR_INVALID
    assert K.enabled(e)[1].height == 8
    assert K.disable(e) == 0 and K.enabled(e)[0] == 0
    assert K.tensor(e, K.DEPTH)[0] == K.ERR_INVALID
    e.set_actions(T.mpenv_tape.tape_actions(1234, 0, 0, 2))
    e.step()  # a step with the camera off again
    # another size
    big = K.config(24, 16, 100.0)
    assert K.enable(e, big) == 0
    assert K.tensor(e, K.DEPTH)[3] == (2, 16, 24)
    e.set_actions(T.mpenv_tape.tape_actions(1234, 1, 0, 2))
    e.step()
    K.check_images(e, K.expected(big, *K.agent_state(e), 2), "in-step image after re-enable at another size")
    e.close()


def test_direct_gpu_stream_step_still_renders():
    import torch

    name = "3x3v3_16x8"
    c = K.CONFIGS[name]
    cfg, tape, steps, posed = K.plan(name)
    want = dict(steps)
    e = engine(name)
    stream = torch.cuda.Stream()
    sb = T.StreamBuffers(e, n_sets=1)
    torch.cuda.synchronize()
    e.gpu_stream_init(stream.cuda_stream, sb.arrs[0])
    stream.synchronize()
    K.check_images(e, want[-1], "after gpuStreamInit")
    for s in range(4):
        sb.set_actions(0, tape[s])
        torch.cuda.synchronize()
        e.gpu_stream_step(stream.cuda_stream, sb.arrs[0])
        stream.synchronize()
    K.check_images(e, want[3], "after four direct gpuStreamSteps")
    e.close()


def test_python_surface():
    import torch

    import madrona_mp_env as m

    name = "3x3v3_16x8"
    c = K.CONFIGS[name]
    cfg, tape, steps, posed = K.plan(name)
    sim = m.SimManager(exec_mode=m.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=c["W"], rand_seed=5, auto_reset=True,
                       sim_flags=int(m.SimFlags.Default), task_type=m.Task.Zone, team_size=c["team"],
                       num_pbt_policies=0, policy_history_size=0, scene_path=T.SCENE)
    ctrl = sim.sim_control_tensor().to_torch()
    ctrl.copy_(torch.tensor([0, 1, 1], dtype=torch.int32, device=ctrl.device).view_as(ctrl))
    assert sim.camera_config() is None
    with pytest.raises(RuntimeError, match="disabled"):
        sim.camera_depth()
    with pytest.raises(RuntimeError, match="width"):
        sim.enable_camera(12, 8)
    sim.enable_camera(16, 8)
    assert sim.camera_config() == (16, 8, 90.0)
    sim.init()
    depth, label = sim.camera_depth().to_torch(), sim.camera_label().to_torch()
    assert depth.dtype == torch.float32 and label.dtype == torch.uint8
    assert tuple(depth.shape) == tuple(label.shape) == (18, 8, 16) and sim.camera_label().dtype == "uint8"
    exp = dict(steps)[-1]
    T.compare(depth.cpu().numpy(), exp[0], "camera_depth() after init")
    T.compare(label.cpu().numpy(), exp[1], "camera_label() after init")
    # zero-copy: the same tensors show the next render
    depth.zero_()
    sim.render_camera()
    T.compare(depth.cpu().numpy(), exp[0], "camera_depth() after render_camera()")
    sim.disable_camera()
    assert sim.camera_config() is None
