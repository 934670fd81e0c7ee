"""k_lidar's task scheduling (csrc/lidar.hip): a block's waves draw its
tasks from a counter in LDS, the stream path's caller-buffer pointers are
read once per block, and `iters` (wave tasks per wave of a block) is chosen
per batch or forced with mpenv_set_lidar_iters.  None of it may change an
output byte: everything here is compared bit for bit, with the oracle or
between runs.
"""
import numpy as np
import pytest

import mpenv_testlib as T

pytestmark = pytest.mark.gpu

LIDAR_EXPORTS = ["FWD_LIDAR", "REAR_LIDAR", "FULL_TEAM_FWD_LIDAR", "FULL_TEAM_REAR_LIDAR"]


# (team size, worlds, forced iters); tasks = ceil(A / 4) * 5, 16 * iters per block
#   (1, 3, 1):  A = 6: a tail unit with two valid agents, rear groups partly invalid
#   (3, 5, 2):  A = 30: units straddle worlds, 40 tasks in two blocks of 32 (the
#               boundary splits unit 6 between its forward tasks and its rear
#               task), half-valid tail unit, T < 6: full-team slots != agent indices
#   (6, 3, 2):  A = 36: 45 tasks, block boundary inside a unit
#   (6, 3, 12): one block, 45 tasks drawn by 16 waves
@pytest.mark.parametrize("ts,W,iters", [(1, 3, 1), (3, 5, 2), (6, 3, 2), (6, 3, 12)])
def test_lidar_sched_oracle_parity(ts, W, iters):
    A = W * 2 * ts
    e = T.Engine(W, ts)
    o = T.Oracle(W, ts)
    assert e.set_lidar_iters(iters) == 0, e.lib.mpenv_last_error().decode()
    e.put_ctrl([0, 1, 1])
    o.put_ctrl([0, 1, 1])
    e.init()
    o.init()
    for name in T.STEP_OUTPUTS:
        T.compare(e.get(name), o.get(name), f"{name} after init ({ts}v{ts} x {W}, iters {iters})")
    for s in range(12):
        if s == 6:
            e.trigger_reset(1)
            o.view("RESET")[1] = 1
        acts = T.mpenv_tape.tape_actions(1234, s, 0, A)
        e.set_actions(acts)
        o.set_actions(acts)
        e.step()
        o.step()
        for name in T.STEP_OUTPUTS:  # FWD_LIDAR, REAR_LIDAR, FULL_TEAM_FWD_LIDAR, FULL_TEAM_REAR_LIDAR among them
            T.compare(e.get(name), o.get(name), f"{name} @ step {s} ({ts}v{ts} x {W}, iters {iters})")
    e.close()
    o.close()


def test_lidar_iters_do_not_change_a_byte():
    """6v6 x 64 worlds (960 wave tasks), 8 steps: runs with iters forced to
    1, 2, 6 and 12 give the automatic run's bytes in every trainInterface
    output and the four lidar exports.  Then, on one engine, every change of
    the value re-captures the step graph once (it is a kernel argument), the
    graph stays on, and the re-captured steps still give the same bytes."""
    ts, W, steps = 6, 64, 8
    A = W * 2 * ts
    names = sorted(set(T.TRAIN_OUTPUTS.values()) | set(LIDAR_EXPORTS))
    forced = (1, 2, 6, 12)
    auto = T.Engine(W, ts)
    runs = {n: T.Engine(W, ts) for n in forced}
    for n, e in runs.items():
        assert e.set_lidar_iters(n) == 0, e.lib.mpenv_last_error().decode()
    for e in [auto] + list(runs.values()):
        e.put_ctrl([0, 1, 1])
        e.init()

    def step_all(s, engines):
        acts = T.mpenv_tape.tape_actions(1234, s, 0, A)
        for e in engines:
            e.set_actions(acts)
            e.step()

    def check(s, engines):
        want = {name: auto.get(name) for name in names}
        for n, e in engines.items():
            for name in names:
                T.compare(e.get(name), want[name], f"{name} @ step {s}: iters {n} against the automatic run")

    for s in range(steps):
        step_all(s, [auto] + list(runs.values()))
        check(s, runs)
    # one engine, the value changed between steps
    ref = {12: runs[12]}
    c0 = auto.graph_captures()
    assert c0 >= 1 and auto.graph_status()[0], auto.graph_status()
    for k, n in enumerate((1, 2, 6, 12, 0)):
        assert auto.set_lidar_iters(n) == 0, auto.lib.mpenv_last_error().decode()
        for rep in range(2):  # the second step with the same value replays the graph
            step_all(steps + 2 * k + rep, [auto, runs[12]])
            assert auto.graph_captures() == c0 + k + 1, (n, rep, auto.graph_captures(), c0)
        check(steps + 2 * k + 1, ref)
    assert auto.graph_status() == (True, ""), auto.graph_status()
    for e in [auto] + list(runs.values()):
        e.close()


def test_lidar_iters_out_of_range():
    e = T.Engine(4, 2)
    for n in (-1, 13, 1 << 20):
        assert e.set_lidar_iters(n) != 0
        assert "lidar iters" in e.lib.mpenv_last_error().decode()
    assert e.set_lidar_iters(12) == 0 and e.set_lidar_iters(0) == 0
    e.close()

    import madrona_mp_env as m

    sim = m.SimManager(exec_mode=m.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=4, rand_seed=5,
                       auto_reset=True, sim_flags=int(m.SimFlags.Default), task_type=m.Task.Zone,
                       team_size=2, num_pbt_policies=0, policy_history_size=0, scene_path=T.SCENE)
    sim.set_lidar_iters(3)
    with pytest.raises(Exception, match="lidar iters"):
        sim.set_lidar_iters(13)


def test_lidar_sched_stream_path():
    """gpuStreamStep with multi-task blocks (3v3 x 5 worlds, iters 2): k_lidar
    writes the lidar rows into the call's buffers too and zero-fills the two
    agent maps there, from pointers it reads once per block.  Two caller
    buffer sets alternate; their lidar and agent-map buffers hold NaNs before
    each step.  Afterwards a plain step writes the engine's own exports."""
    import torch

    ts, W, iters = 3, 5, 2
    A = W * 2 * ts
    e = T.Engine(W, ts)
    o = T.Oracle(W, ts)
    assert e.set_lidar_iters(iters) == 0, e.lib.mpenv_last_error().decode()
    sb = T.StreamBuffers(e)
    sets, arrs, idx = sb.sets, sb.arrs, sb.idx
    maps = ("agent_map", "unmasked_agent_map")
    nan_filled = ("fwd_lidar", "rear_lidar") + maps
    o.put_ctrl([0, 1, 1])
    e.put_ctrl([0, 1, 1])
    stream = torch.cuda.Stream()
    e.gpu_stream_init(stream.cuda_stream, arrs[0])
    o.init()
    stream.synchronize()
    for s in range(6):
        bufs = sets[s % 2]
        acts = T.mpenv_tape.tape_actions(1234, s, 0, A)
        sb.set_actions(s % 2, acts)
        for nm in nan_filled:
            bufs[idx[nm]].fill_(float("nan"))
        torch.cuda.synchronize()
        e.gpu_stream_step(stream.cuda_stream, arrs[s % 2])
        o.set_actions(acts)
        o.step()
        stream.synchronize()
        for (io, nm, ename, _, _), b in zip(sb.ti, bufs):
            if io != 1:
                continue
            got = b.cpu().numpy()
            if nm in maps:
                assert got.shape[0] == A and (got.view(np.uint32) == 0).all(), f"{nm} @ {s}: not all zero"
            else:
                T.compare(got, o.get(ename), f"{ename} ({nm}) in the caller's buffer @ {s}")
        # the engine's own lidar is state (the next full-team copy reads it)
        for name in LIDAR_EXPORTS:
            T.compare(e.get(name), o.get(name), f"{name} engine export @ {s}")
    acts = T.mpenv_tape.tape_actions(1234, 6, 0, A)
    e.set_actions(acts)
    e.step()
    o.set_actions(acts)
    o.step()
    for (io, nm, ename, _, _) in sb.ti:
        if io == 1 and nm not in maps:
            T.compare(e.get(ename), o.get(ename), f"engine export {ename} after the stream steps")
    for name in LIDAR_EXPORTS:
        T.compare(e.get(name), o.get(name), f"{name} after the stream steps")
    e.close()
    o.close()
