"""gpuStreamStep (Manager::gpuStreamInit / gpuStreamStep, mgr.cpp:507-645) at
ragged shapes, against the oracle bit for bit.

tests/test_parity_gpu.py::test_gpu_stream_step_buffers_abi runs 2v2 x 16,
where every copied segment is a multiple of 16 B, every buffer is aligned and
every world group starts on a 4-agent boundary.  Here: 1v1 x 3, 3v3 x 5 and
5v5 x 3, whose [W] and [A] segments are 12, 20, 24 and 120 B (k_copy_batch's
partial last piece, and segments without one whole 16-B piece), in world
groups whose first agent is 2, 6 or 10 (the direct path's destinations
offset by outBase off a 4-agent boundary); one direct output handed in 4 B
into its allocation (directTable must fall back to copying, copyTI to
hipMemcpyAsync for that buffer); and a null output pointer (skipped).

Shapes are (team size, worlds, world groups)."""
import numpy as np
import pytest

import mpenv_testlib as T

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 1), (1, 3, 3), (3, 5, 3), (5, 3, 2)]
STEPS = 30
SEED = 1234
# the outputs k_obs / k_lidar write straight into the caller's buffers
# (csrc/manager.cpp kTIOutputs `direct`); every other output, and every input,
# is a copied segment
DIRECT = {"fwd_lidar", "rear_lidar", "self", "filters_state", "teammates", "opponents", "self_pos",
          "teammate_positions", "opponent_positions", "opponent_masks", "agent_map", "unmasked_agent_map"}


def run(ts, W, groups, offset_output=None, null_output=None):
    """The structure of test_gpu_stream_step_buffers_abi: two caller buffer
    sets alternate, outputs pre-filled with 7, every output of the set a step
    used equals the oracle's; the capture count stays; a plain step()
    afterwards writes the engine's exports again.

    offset_output: that output of both sets is a view 4 B into a larger
    allocation.  null_output: that output's pointer is passed as null; its
    buffer must keep its 7s."""
    import torch

    A = W * 2 * ts
    e = T.Engine(W, ts)
    o = T.Oracle(W, ts)
    if groups > 1:
        e.set_world_groups(groups)
    sb = T.StreamBuffers(e)
    ti, sets, idx = sb.ti, sb.sets, sb.idx
    names = [nm for _, nm, _, _, _ in ti]
    assert DIRECT <= set(names) and offset_output in DIRECT | {None} and null_output not in DIRECT
    # what the copies are made of, from the export descriptors: a segment with
    # a partial last 16-B piece, and one without a whole piece
    copied = [int(np.prod(shape)) * 4 for io, nm, _, _, shape in ti if nm not in DIRECT]
    assert any(b % 16 != 0 for b in copied), copied
    assert any(b < 16 for b in copied), copied
    if groups > 1:  # some group's first agent is off the 4-agent boundary
        assert any((W * i // groups * 2 * ts) % 4 for i in range(1, groups))

    for bs in sets:
        assert all(t.data_ptr() % 16 == 0 for t in bs)
        if offset_output:
            t = bs[idx[offset_output]]
            whole = torch.full((t.numel() + 4,), 7, dtype=t.dtype, device="cuda")
            bs[idx[offset_output]] = whole[1:t.numel() + 1].view(t.shape)
            assert bs[idx[offset_output]].data_ptr() % 16 == 4
    sb.point()
    arrs = sb.arrs
    if null_output:
        for arr in arrs:
            arr[idx[null_output]] = None
    o.put_ctrl([0, 1, 1])
    e.put_ctrl([0, 1, 1])
    stream = torch.cuda.Stream()
    e.gpu_stream_init(stream.cuda_stream, arrs[0])
    o.init()
    stream.synchronize()

    def check(bufs, where):
        for (io, nm, ename, _, _), b in zip(ti, bufs):
            if io == 0:
                continue
            got = b.cpu().numpy()
            if nm == null_output:
                assert (got == 7).all(), f"{nm} was passed as null and written @ {where}"
            else:
                T.compare(got, o.get(ename), f"{nm} @ {where}")

    check(sets[0], "init")
    caps = []
    for s in range(STEPS):
        bufs = sets[s % 2]
        acts = T.mpenv_tape.tape_actions(SEED, s, 0, A)
        sb.set_actions(s % 2, acts)
        torch.cuda.synchronize()
        e.gpu_stream_step(stream.cuda_stream, arrs[s % 2])
        o.set_actions(acts)
        o.step()
        stream.synchronize()
        check(bufs, f"step {s}")
        caps.append(e.graph_captures())
    assert caps[0] >= 1 and caps[-1] == caps[0], caps  # one capture serves both buffer sets
    if offset_output:  # the guard elements around the offset view are untouched
        for bs in sets:
            t = bs[idx[offset_output]]
            base = t._base if t._base is not None else t
            flat = base.reshape(-1).cpu().numpy()
            n = t.numel()
            assert flat[0] == 7 and (flat[n + 1:] == 7).all(), offset_output
    # a plain step afterwards: the engine's own exports are written again
    acts = T.mpenv_tape.tape_actions(SEED, STEPS, 0, A)
    e.set_actions(acts)
    e.step()
    o.set_actions(acts)
    o.step()
    for io, nm, ename, _, _ in ti:
        if io == 1 and nm not in ("agent_map", "unmasked_agent_map"):
            T.compare(e.get(ename), o.get(ename), f"engine export {nm} after the stream steps")
    e.close()
    o.close()


@pytest.mark.parametrize("ts,W,groups", SHAPES)
def test_gpu_stream_step_at_ragged_shapes(ts, W, groups):
    run(ts, W, groups)


def test_gpu_stream_step_copies_when_a_direct_output_is_unaligned():
    run(3, 5, 3, offset_output="self_pos")


def test_gpu_stream_step_skips_a_null_output():
    run(3, 5, 3, null_output="hp")
