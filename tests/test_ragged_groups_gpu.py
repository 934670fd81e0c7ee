"""The step path with world groups that start off a 4-agent boundary, against
the oracle bit for bit.

sliceState (csrc/manager.cpp) gives every world group pointers offset by
g0 = w0 * N agents.  With N = 4 or 12, or an even first world, g0 is a multiple
of 4 agents and every per-agent span of a group starts 16-B aligned like the
whole batch; with N in {2, 6, 10} and an odd first world it does not, and
k_obs's HalfStage::flushSpan takes its scalar branch.  Every other multi-group
test of the suite is aligned (2v2 x 2050, 3v3 x 3000 at worlds 1000 / 1500 /
2000, 3v3 x 12 in three groups, 6v6 x 7), so these shapes are the only ones
that run that branch, and the only ones that would see any other kernel
assume a group's pointers keep the batch's alignment.  6v6 x 7 in three groups
is the aligned control.

Shapes are (team size, worlds, world groups); groups split at W * i / groups
(mpenv_manager::setupGroups)."""
import numpy as np
import pytest

import mpenv_testlib as T

pytestmark = pytest.mark.gpu

# (team size, worlds, groups): first worlds of groups 1.., as the split gives them
SHAPES = {
    (1, 3, 3): [1, 2],
    (3, 5, 3): [1, 3],
    (5, 3, 2): [1],
    (5, 15, 2): [7],     # groups of 70 and 80 agents: two waves each, the second partial
    (3, 23, 3): [7, 15],
    (6, 7, 3): [2, 4],   # the aligned control
}
CONTROL = (6, 7, 3)
NAMES = T.STEP_OUTPUTS + T.DEBUG_OUTPUTS
# 60 steps; 3v3 x 5 and 5v5 x 3 need longer for the coverage asserted below:
# with seed 5 the oracle's first lidar ray that hits nothing comes at step 62
# (3v3 x 5) and 74 (5v5 x 3); at the other shapes every class is there by step 41
STEPS = {(3, 5, 3): 120, (5, 3, 2): 120}
# floats per agent of three spans k_obs flushes: self position, self
# observation, teammate positions
SPAN_FLOATS = (3, 43, 15)


def group_starts(W, groups):
    return [W * i // groups for i in range(1, groups)]


def misaligned_spans(ts, W, groups):
    """{n: some group's first agent g0 has g0 * n * 4 % 16 != 0}"""
    N = 2 * ts
    return {n: any((w0 * N * n * 4) % 16 != 0 for w0 in group_starts(W, groups)) for n in SPAN_FLOATS}


def lidar_classes(o):
    """the set of classes (0 none, 1 wall, 2 teammate, 3 opponent) in the oracle's lidar"""
    rows = np.concatenate([o.get("FWD_LIDAR").reshape(-1, 4), o.get("REAR_LIDAR").reshape(-1, 4)])
    cls = np.where(rows[:, 1] == 1, 1, np.where(rows[:, 2] == 1, 2, np.where(rows[:, 3] == 1, 3, 0)))
    assert (rows[cls == 0] == np.array([-1, 0, 0, 0], np.float32)).all()
    return set(int(c) for c in np.unique(cls))


@pytest.mark.parametrize("ts,W,groups", list(SHAPES), ids=[f"{t}v{t}x{w}g{g}" for t, w, g in SHAPES])
def test_misaligned_world_groups_match_the_oracle(monkeypatch, ts, W, groups):
    shape = (ts, W, groups)
    N = 2 * ts
    steps = STEPS.get(shape, 60)
    # the shape does what this test is for (from the shape, not from the engine)
    assert group_starts(W, groups) == SHAPES[shape]
    mis = misaligned_spans(ts, W, groups)
    if shape == CONTROL:
        assert not any(mis.values()), mis
    else:
        assert all(mis.values()), mis

    # one engine launching kernel by kernel, one replaying the captured step graph
    monkeypatch.setenv("MPENV_STEP_GRAPH", "0")
    direct = T.Engine(W, ts, sim_flags=1)
    monkeypatch.setenv("MPENV_STEP_GRAPH", "1")
    graph = T.Engine(W, ts, sim_flags=1)
    engines = {"direct launches": direct, "step graph": graph}
    o = T.Oracle(W, ts, sim_flags=1)
    for e in engines.values():
        e.set_world_groups(groups)
        e.put_ctrl([0, 1, 1])
        e.init()
    o.put_ctrl([0, 1, 1])
    o.init()
    classes = set()
    masks = lk_obs = lk_pos = False
    for s in range(steps):
        acts = T.combat_actions(o, s)
        o.set_actions(acts)
        o.step()
        want = {n: o.get(n) for n in NAMES}
        want_cells = T.explore_visited(o)
        for how, e in engines.items():
            e.set_actions(acts)
            e.step()
            for n in NAMES:
                T.compare(e.get(n), want[n], f"{n} ({how}) @ {s}")
            T.compare(T.explore_visited(e), want_cells, f"explore cells ({how}) @ {s}")
        classes |= lidar_classes(o)
        masks = masks or bool(want["OPPONENT_MASKS"].any())
        lk_obs = lk_obs or bool(want["OPPONENT_LAST_KNOWN_OBSERVATIONS"].any())
        lk_pos = lk_pos or bool(want["OPPONENT_LAST_KNOWN_POSITIONS"].any())
    # what the run reached, from the oracle alone
    assert classes == ({0, 1, 3} if ts == 1 else {0, 1, 2, 3}), classes
    assert masks and lk_obs and lk_pos
    caps = direct.graph_captures(), graph.graph_captures()
    assert caps == (0, 1), caps
    for e in engines.values():
        e.close()
    o.close()
