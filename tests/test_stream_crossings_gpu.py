"""gpuStreamStep crossed with the features that read what it leaves behind:
the engine's own exports, checkpoints, the device aim-bot, the wire sender,
world groups and triggered resets, against the oracle bit for bit.

A direct mpenv_gpu_stream_step (every direct output present and 16-B aligned,
no policy loaded) has k_obs write the eight observation exports (OBS8 below)
into the caller's buffers only; the engine's own rows keep their content.
Every other export is state the step itself reads and stays current.  What
reads the stale rows -- mpenv_combat_actions, mpenv_state_save,
mpenv_policy_load (tests/test_policy_gpu.py) -- is refused until a plain step
or a copying stream step has written them again.

Shapes are (team size, worlds, world groups): (1, 3, 3), (3, 5, 3) and
(5, 3, 2) start world groups off the 4-agent boundary
(tests/test_ragged_groups_gpu.py); (6, 7, 3) is the aligned control.  The
oracle runs each (team size, worlds) once, with sim_flags 1 and the numpy
aim-bot (T.combat_actions) on its own observations, and records its outputs
and the actions it played; the tests share the record and do not modify it.

A stale read shows only if the rows moved: wherever a test claims that a call
would have read stale rows, moved_since() asserts from the oracle's record
alone that the masks are non-zero and that masks, opponent rows and self rows
differ from their values at the engine's last plain step."""
import functools

import numpy as np
import pytest
import torch  # before the oracle loads libmpenv.so: with the order reversed torch finds no GPU

import mpenv_testlib as T

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 3), (3, 5, 3), (5, 3, 2), (6, 7, 3)]
RAGGED = [(3, 5, 3), (5, 3, 2)]
SEED = 1234
RUN = 48  # recorded oracle steps per shape
ERR_INVALID = -1
# the exports k_obs writes through OutTab (csrc/manager.cpp kTIOutputs `direct`, less the lidar)
OBS8 = ["OPPONENT_MASKS", "FILTERS_STATE", "SELF_OBSERVATION", "TEAMMATE_OBSERVATIONS", "OPPONENT_OBSERVATIONS",
        "SELF_POSITION", "TEAMMATE_POSITIONS", "OPPONENT_POSITIONS"]
ALL = T.STEP_OUTPUTS + T.DEBUG_OUTPUTS + ["EXPLORE"]
STATE_BACKED = [n for n in ALL if n not in OBS8]
assert len(OBS8) == 8 and len(STATE_BACKED) == len(ALL) - 8
for must in ("HP", "MAGAZINE", "ALIVE", "REWARD", "DONE", "MATCH_RESULT", "FWD_LIDAR", "REAR_LIDAR",
             "OPPONENT_LAST_KNOWN_OBSERVATIONS", "OPPONENT_LAST_KNOWN_POSITIONS", "FULL_TEAM_FWD_LIDAR",
             "FULL_TEAM_REAR_LIDAR", "DEBUG_AGENT_F32", "DEBUG_WORLD_I32"):
    assert must in STATE_BACKED


def outputs(sim, names=ALL):
    return {n: T.explore_visited(sim) if n == "EXPLORE" else sim.get(n) for n in names}


def tape(step, A):
    return T.mpenv_tape.tape_actions(SEED, step, 0, A)


class Recorded:
    """One recorded step as T.combat_actions / T.seek_combat_actions take a sim."""

    def __init__(self, W, N, out):
        self.W, self.N, self.out = W, N, out

    def get(self, name):
        return self.out[name]


@functools.lru_cache(maxsize=None)
def oracle_run(ts, W, auto_reset=True, resets=()):
    """{"init": outputs, s: outputs after step s, "acts": [actions of step s]}
    for s in 0..RUN-1; resets = ((step, world), ...) are triggered before that
    step.  Computed once per argument set; the arrays are read-only."""
    o = T.Oracle(W, ts, sim_flags=1, auto_reset=auto_reset)
    o.put_ctrl([0, 1, 1])
    o.init()
    rec = {"init": outputs(o), "acts": []}
    for s in range(RUN):
        acts = T.combat_actions(o, s, SEED)
        for at, w in resets:
            if at == s:
                o.view("RESET")[w] = 1
        o.set_actions(acts)
        o.step()
        rec["acts"].append(acts)
        rec[s] = outputs(o)
    assert not o.get("AGENT_MAP").any()  # never written: the callers' agent maps are zero fills
    o.close()
    for k, d in rec.items():
        for a in (d if k == "acts" else d.values()):
            a.setflags(write=False)
    return rec


def differs(rec, plain, step, name):
    return bool((rec[step][name].view(np.uint32) != rec[plain][name].view(np.uint32)).any())


def moved_since(rec, plain, step):
    """The condition on a staleness assertion, from the oracle's record alone:
    at `step` an opponent is visible somewhere, and masks, opponent rows and
    self rows differ from the engine's last plain step (or "init")."""
    assert rec[step]["OPPONENT_MASKS"].any(), step
    for n in ("OPPONENT_MASKS", "OPPONENT_OBSERVATIONS", "SELF_OBSERVATION"):
        assert differs(rec, plain, step, n), (n, plain, step)


def same_bytes(got, want, what):
    for n in want:
        assert got[n].tobytes() == want[n].tobytes(), f"{n}: {what}"


class Rig:
    """An engine (sim_flags 1) with two caller buffer sets on a side stream,
    after gpu_stream_init into set 0."""

    def __init__(self, ts, W, groups=1, offset_output=None, **kw):
        self.e = T.Engine(W, ts, sim_flags=1, **kw)
        self.A = W * 2 * ts
        if groups > 1:
            self.e.set_world_groups(groups)
        self.sb = T.StreamBuffers(self.e)
        self.offset_set = None
        if offset_output:
            # a third pointer array: set 0 with one direct output 4 B into a
            # larger allocation, which sends the whole call down the copy path
            i = self.sb.idx[offset_output]
            t = self.sb.sets[0][i]
            self.whole = torch.full((t.numel() + 4,), 7, dtype=t.dtype, device="cuda")
            self.offset_view = self.whole[1:t.numel() + 1].view(t.shape)
            assert self.offset_view.data_ptr() % 16 == 4
            arr = type(self.sb.arrs[0])(*self.sb.arrs[0])
            arr[i] = self.offset_view.data_ptr()
            self.offset_set = (arr, i)
        self.stream = torch.cuda.Stream()
        self.e.put_ctrl([0, 1, 1])
        torch.cuda.synchronize()
        self.e.gpu_stream_init(self.stream.cuda_stream, self.sb.arrs[0])
        self.stream.synchronize()
        self.n_stream = 0
        self.zeros_resets = np.zeros(W, np.int32)

    def stream_step(self, acts, k=None, resets=None, copying=False):
        """One gpu_stream_step with buffer set k (default: the sets alternate);
        returns k.  copying: through the pointer array with the offset output."""
        if k is None:
            k = 0 if copying else self.n_stream % 2
        self.n_stream += 1
        self.sb.set_actions(k, acts)
        self.sb.put(k, "resets", self.zeros_resets if resets is None else resets)
        torch.cuda.synchronize()
        arr = self.offset_set[0] if copying else self.sb.arrs[k]
        self.e.gpu_stream_step(self.stream.cuda_stream, arr)
        self.stream.synchronize()
        return k

    def plain_step(self, acts):
        self.e.set_actions(acts)
        self.e.step()

    def buffers(self, k, copying=False):
        """{export name: array} of set k's outputs (the agent maps apart)"""
        out, maps = {}, []
        for i, ((io, nm, ename, _, _), b) in enumerate(zip(self.sb.ti, self.sb.sets[k])):
            if io == 0:
                continue
            if copying and i == self.offset_set[1]:
                b = self.offset_view
            if "agent_map" in nm:
                maps.append(b)
            else:
                out[ename] = b.cpu().numpy()
        assert len(maps) == 2
        return out, maps

    def check_buffers(self, k, want, where, copying=False):
        got, maps = self.buffers(k, copying)
        assert set(got) == set(T.TRAIN_OUTPUTS.values())
        for n in got:
            T.compare(got[n], want[n], f"caller's {n} @ {where}")
        for t in maps:
            assert not t.any().item(), f"agent map not zero-filled @ {where}"

    def check_engine(self, want, where, names=ALL):
        got = outputs(self.e, names)
        for n in names:
            T.compare(got[n], want[n], f"engine's {n} @ {where}")

    def check_after_direct(self, k, want, obs_before, where):
        """(a): the caller's buffers and the engine's state-backed exports
        equal the oracle; the engine's observation rows hold what they held."""
        self.check_buffers(k, want, where)
        self.check_engine(want, where, STATE_BACKED)
        same_bytes(outputs(self.e, OBS8), obs_before, f"written by a direct stream step @ {where}")

    def close(self):
        self.e.close()


# ------------------------------------------------ a: the engine's rows after a direct step

@pytest.mark.parametrize("ts,W,groups", SHAPES)
def test_engine_rows_after_direct_stream_steps(ts, W, groups):
    rec = oracle_run(ts, W)
    steps = 30
    moved_since(rec, "init", 0)          # the very first step already moves the rows
    moved_since(rec, "init", steps - 1)
    r = Rig(ts, W, groups)
    r.check_buffers(0, rec["init"], "init")
    r.check_engine(rec["init"], "init")
    obs_init = outputs(r.e, OBS8)
    caps = []
    for s in range(steps):
        k = r.stream_step(rec["acts"][s])
        assert k == s % 2
        r.check_after_direct(k, rec[s], obs_init, f"step {s}")
        caps.append(r.e.graph_captures())
    assert caps[0] >= 1 and len(set(caps)) == 1, caps
    r.close()


# ------------------------------------------------ b: plain and stream steps interleaved

def interleaving(n=40, seed=3):
    pat = "".join("PS"[b] for b in np.random.default_rng(seed).integers(0, 2, n))
    pairs = [pat[i:i + 2] for i in range(n - 1)]
    return pat, {p: pairs.count(p) for p in ("PS", "SP", "SS", "PP")}


@pytest.mark.parametrize("ts,W,groups", SHAPES)
def test_plain_and_stream_steps_interleaved(ts, W, groups):
    rec = oracle_run(ts, W)
    pat, pairs = interleaving()
    assert min(pairs.values()) >= 3, pairs
    r = Rig(ts, W, groups)
    obs = outputs(r.e, OBS8)
    last_plain = "init"
    caps, seen = [], set()
    # "untouched" tells only where the rows moved.  The self rows move at every
    # step; the masks of a small batch repeat now and then (1v1 x 3 has 6 mask
    # rows), so all three kinds of row moving is asked of three stream steps
    # after a plain step and three after a stream step, not of every one.
    moved = {"P": 0, "S": 0}
    for s, kind in enumerate(pat):
        if kind == "P":
            r.plain_step(rec["acts"][s])
            r.check_engine(rec[s], f"plain step {s} ({pat[:s + 1]})")
            obs = outputs(r.e, OBS8)
            last_plain = s
        else:
            assert differs(rec, last_plain, s, "SELF_OBSERVATION"), s
            if all(differs(rec, last_plain, s, n) for n in ("OPPONENT_MASKS", "OPPONENT_OBSERVATIONS")):
                assert rec[s]["OPPONENT_MASKS"].any()
                moved[pat[s - 1] if s else "P"] += 1
            k = r.stream_step(rec["acts"][s])
            r.check_after_direct(k, rec[s], obs, f"stream step {s} ({pat[:s + 1]})")
        seen.add(kind)
        if seen == {"P", "S"}:
            caps.append(r.e.graph_captures())
    assert min(moved.values()) >= 3, moved
    assert len(caps) > 30 and caps[0] >= 1 and len(set(caps)) == 1, caps
    r.close()


# ------------------------------------------------ c: the device aim-bot

def aimbot(r, step, mode, out):
    """mpenv_combat_actions over the tape row of `step` into the device buffer
    `out` (pre-filled with -7); returns (status, out's content)."""
    A = r.A
    dtape = r.e.mem.upload(tape(step, A))
    r.e.mem.h2d(out, np.full((A, 6), -7, np.int32))
    rc = r.e.lib.mpenv_combat_actions(r.e.h, dtape, out, mode, None)
    r.e.mem.hip.hipDeviceSynchronize()
    got = np.empty((A, 6), np.int32)
    r.e.mem.d2h(out, got.nbytes, got)
    r.e.mem.free(dtape)
    return rc, got


def twin(rec, ts, W, step, mode, rows_of=None):
    """The numpy aim-bot's actions for `step`: the tape row of `step` over the
    oracle's observations after step `step - 1` (or after step rows_of)."""
    fn = T.seek_combat_actions if mode else T.combat_actions
    rows = rec[step - 1 if rows_of is None else rows_of]
    return fn(Recorded(W, 2 * ts, rows), step, base=tape(step, W * 2 * ts))


def assert_refused(e, rc, who):
    assert rc == ERR_INVALID, (who, rc)
    why = e.lib.mpenv_last_error().decode()
    assert "mpenv_gpu_stream_step" in why and who in why, why


@pytest.mark.parametrize("ts,W,groups", SHAPES)
def test_device_aimbot_is_refused_on_stale_rows_and_right_on_current_ones(ts, W, groups):
    rec = oracle_run(ts, W)
    r = Rig(ts, W, groups, offset_output="self_pos")
    e, A = r.e, r.A
    out = e.mem.upload(np.zeros((A, 6), np.int32))
    plain, direct = 2, 8
    for s in range(plain + 1):
        r.plain_step(rec["acts"][s])
    for s in range(plain + 1, direct + 1):
        r.stream_step(rec["acts"][s])
    # after a direct step: it would have aimed at the opponents of step `plain`
    moved_since(rec, plain, direct)
    for mode in (0, 1):  # and the twin itself tells the two steps' rows apart
        assert (twin(rec, ts, W, direct + 1, mode) != twin(rec, ts, W, direct + 1, mode, rows_of=plain)).any()
    cols = outputs(e, ["PVP_DISCRETE_ACTION", "PVP_DISCRETE_AIM_ACTION"])
    for mode in (0, 1):
        rc, got = aimbot(r, direct + 1, mode, out)
        assert_refused(e, rc, "mpenv_combat_actions")
        assert (got == -7).all(), f"a refused call wrote its out buffer (mode {mode})"
        dtape = e.mem.upload(tape(direct + 1, A))
        rc = e.lib.mpenv_combat_actions(e.h, dtape, None, mode, None)  # the fused form: into the step inputs
        e.mem.hip.hipDeviceSynchronize()
        e.mem.free(dtape)
        assert_refused(e, rc, "mpenv_combat_actions")
    same_bytes(outputs(e, list(cols)), cols, "a refused aim-bot call wrote the engine's action columns")
    # a copying step (one direct output unaligned) keeps every row current
    s = direct + 1
    k = r.stream_step(rec["acts"][s], copying=True)
    r.check_buffers(k, rec[s], f"copying step {s}", copying=True)
    r.check_engine(rec[s], f"copying step {s}")
    assert r.whole[0].item() == 7 and (r.whole[-3:] == 7).all().item()  # the guard elements
    for mode in (0, 1):
        rc, got = aimbot(r, s + 1, mode, out)
        assert rc == 0, e.lib.mpenv_last_error().decode()
        np.testing.assert_array_equal(got, twin(rec, ts, W, s + 1, mode), err_msg=f"copy path, mode {mode}")
    # refused again after the next direct step, accepted after a plain step
    s += 1
    r.stream_step(rec["acts"][s])
    moved_since(rec, s - 1, s)
    rc, got = aimbot(r, s + 1, 0, out)
    assert_refused(e, rc, "mpenv_combat_actions")
    assert (got == -7).all()
    s += 1
    r.plain_step(rec["acts"][s])
    for mode in (0, 1):
        rc, got = aimbot(r, s + 1, mode, out)
        assert rc == 0, e.lib.mpenv_last_error().decode()
        np.testing.assert_array_equal(got, twin(rec, ts, W, s + 1, mode), err_msg=f"after a plain step, mode {mode}")
    e.mem.free(out)
    r.close()


# ------------------------------------------------ d: checkpoints

@pytest.mark.parametrize("ts,W,groups", SHAPES)
def test_state_save_is_refused_after_a_direct_stream_step(ts, W, groups):
    rec = oracle_run(ts, W)
    r = Rig(ts, W, groups)
    e = r.e
    plain, direct = 2, 8
    for s in range(plain + 1):
        r.plain_step(rec["acts"][s])
    for s in range(plain + 1, direct + 1):
        r.stream_step(rec["acts"][s])
    moved_since(rec, plain, direct)  # the blob would have held the rows of step `plain`
    n = e.state_bytes()
    blob = e.new_state_blob()
    rc = e.lib.mpenv_state_save(e.h, blob, None)
    e.mem.hip.hipDeviceSynchronize()
    assert_refused(e, rc, "mpenv_state_save")
    host = np.empty(n, np.uint8)
    e.mem.d2h(blob, n, host)
    assert (host == 0xA5).all(), "a refused save wrote the blob"
    # after a plain step the save is accepted and the blob restores that step
    s = direct + 1
    r.plain_step(rec["acts"][s])
    e.state_save(blob)
    r.plain_step(rec["acts"][s + 1])
    e.state_load(blob)
    r.check_engine(rec[s], f"load of the snapshot of step {s}")
    assert e.state_error() == 0
    e.mem.free(blob)
    r.close()


S0, K = 5, 8  # the snapshot's step; direct stream steps between save and load


def to_snapshot(r, rec):
    """Stream step 0 (the stream path's capture), plain steps 1..S0, the save."""
    r.stream_step(rec["acts"][0])
    for s in range(1, S0 + 1):
        r.plain_step(rec["acts"][s])
    r.check_engine(rec[S0], f"step {S0}")
    caps = (r.e.graph_captures(), r.e.graph_status()[0])
    blob = r.e.new_state_blob()
    r.e.state_save(blob)
    return blob, caps


@pytest.mark.parametrize("ts,W,groups", SHAPES)
def test_load_between_stream_steps_rewinds_the_callers_outputs(ts, W, groups):
    rec = oracle_run(ts, W)
    r = Rig(ts, W, groups)
    e = r.e
    blob, caps = to_snapshot(r, rec)
    first = []
    for s in range(S0 + 1, S0 + K + 1):
        k = r.stream_step(rec["acts"][s])
        r.check_buffers(k, rec[s], f"step {s}")
        first.append((k, r.buffers(k)[0]))
    e.state_load(blob)
    r.check_engine(rec[S0], "directly after the load")
    for j, s in enumerate(range(S0 + 1, S0 + K + 1)):
        k = r.stream_step(rec["acts"][s], k=1 - first[j][0])  # the other buffer set first
        got = r.buffers(k)[0]
        for n in got:
            T.compare(got[n], first[j][1][n], f"caller's {n} @ replayed step {s} (first pass)")
        r.check_buffers(k, rec[s], f"replayed step {s}")
    assert e.state_error() == 0
    assert (e.graph_captures(), e.graph_status()[0]) == caps and caps[1] == 1 and caps[0] >= 1
    e.mem.free(blob)
    r.close()


@pytest.mark.parametrize("ts,W,groups", RAGGED)
def test_mapped_load_between_stream_steps(ts, W, groups):
    """One world rewound, one forked from a world of another group, the rest
    kept: kept worlds continue, the rewound and the forked world follow the
    recorded source world from S0 on, seen through the caller's buffers."""
    rec = oracle_run(ts, W)
    N = 2 * ts
    rewound, fork, src = 1, W - 1, 0
    source = {w: w for w in range(W)}
    source[fork] = src
    moved = (rewound, fork)
    ep_col = 11  # MPENV_DBG_WI_EPISODE_COUNTER
    for s in range(S0 + 1, S0 + K + 1):  # precondition: the fork's source ends no episode in the window
        assert not rec[s]["DONE"][src * N:(src + 1) * N].any(), s
        assert rec[s]["DEBUG_WORLD_I32"][src, ep_col] == rec[S0]["DEBUG_WORLD_I32"][src, ep_col], s
    r = Rig(ts, W, groups)
    e = r.e
    blob, caps = to_snapshot(r, rec)
    for s in range(S0 + 1, S0 + K + 1):
        r.stream_step(rec["acts"][s])
    wmap = np.full(W, -1, np.int32)
    wmap[rewound], wmap[fork] = rewound, src
    dmap = e.mem.upload(wmap)
    e.state_load(blob, dmap)
    for j in range(1, K + 1):
        then, now = S0 + j, S0 + K + j
        acts = np.array(rec["acts"][now])
        for w in moved:
            acts[w * N:(w + 1) * N] = rec["acts"][then][source[w] * N:(source[w] + 1) * N]
        k = r.stream_step(acts)
        got, maps = r.buffers(k)
        for n, g in got.items():
            per = g.shape[0] // W
            assert per * W == g.shape[0] and per in (1, N), (n, g.shape)
            for w in range(W):
                want = rec[then if w in moved else now][n][source[w] * per:(source[w] + 1) * per]
                T.compare(g[w * per:(w + 1) * per], want,
                          f"caller's {n}, world {w} (oracle world {source[w]}) @ step {j} after the load")
        assert not any(t.any().item() for t in maps)
    assert e.state_error() == 0
    assert (e.graph_captures(), e.graph_status()[0]) == caps and caps[1] == 1
    e.mem.free(dmap)
    e.mem.free(blob)
    r.close()


# ------------------------------------------------ f: the wire sender on the stream path

@pytest.mark.parametrize("ts,W,groups", [(3, 5, 3), (6, 7, 3)])
def test_wire_sender_that_only_takes_direct_stream_steps(ts, W, groups):
    """mpenv_wire_pack reads the engine's lidar rows, which a direct step
    keeps current only because k_lidar stores both copies."""
    rec = oracle_run(ts, W)
    steps = 40
    r = Rig(ts, W, groups)
    e = r.e
    plain = T.Engine(W, ts, sim_flags=1)  # the twin sender: plain steps, same actions
    sh = T.Engine(W, ts, sim_flags=1)
    plain.put_ctrl([0, 1, 1])
    plain.init()
    nkey, nmsg = e.wire_bytes(True), e.wire_bytes(False)
    buf = e.mem.upload(np.zeros(nkey, np.uint8))
    buf2 = e.mem.upload(np.zeros(nkey, np.uint8))
    for s in range(steps):
        r.stream_step(rec["acts"][s])
        plain.set_actions(rec["acts"][s])
        plain.step()
        key = s == 0
        n = nkey if key else nmsg
        e.wire_pack(buf, key)
        plain.wire_pack(buf2, key)
        a, b = np.empty(n, np.uint8), np.empty(n, np.uint8)
        e.mem.d2h(buf, n, a)
        e.mem.d2h(buf2, n, b)
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, f"step {s}: {bad.size} message bytes differ from the plain sender's, first at {bad[0]}"
        sh.wire_unpack(buf, key)
        assert sh.wire_error() == 0, s
        for nm, ex in T.TRAIN_OUTPUTS.items():
            T.compare(sh.get(ex), rec[s][ex], f"shadow's {nm} @ step {s}")
    e.mem.free(buf)
    e.mem.free(buf2)
    for x in (plain, sh):
        x.close()
    r.close()


# ------------------------------------------------ g: world groups changed between stream steps

@pytest.mark.parametrize("ts,W", [(3, 5), (5, 3)])
def test_world_groups_changed_between_stream_steps(ts, W):
    rec = oracle_run(ts, W)
    plan = [1, 3, 2, 1]
    assert any((W * i // g * 2 * ts) % 4 for g in plan for i in range(1, g))  # a group start off the boundary
    r = Rig(ts, W, plan[0])
    caps = []
    for s in range(8 * len(plan)):
        if s % 8 == 0 and s:
            r.e.set_world_groups(plan[s // 8])
        k = r.stream_step(rec["acts"][s])
        r.check_buffers(k, rec[s], f"step {s} ({plan[s // 8]} groups)")
        caps.append(r.e.graph_captures())
    for i, g in enumerate(plan):
        seg = caps[8 * i:8 * i + 8]
        assert seg[0] >= 1 and len(set(seg)) == 1, (g, caps)
    r.check_engine(rec[8 * len(plan) - 1], "the last step", STATE_BACKED)
    r.close()


# ------------------------------------------------ h: a triggered reset under the stream path

@pytest.mark.parametrize("ts,W,groups", [(1, 3, 3), (3, 5, 3)])
def test_triggered_resets_through_the_callers_reset_buffer(ts, W, groups):
    resets = ((10, 1), (11, W - 1))
    rec = oracle_run(ts, W, auto_reset=False, resets=resets)
    ep_col = 11  # MPENV_DBG_WI_EPISODE_COUNTER
    for at, w in resets:  # the reset happened in its own step, from the oracle's record
        assert rec[at]["DEBUG_WORLD_I32"][w, ep_col] != rec[at - 1]["DEBUG_WORLD_I32"][w, ep_col]
    r = Rig(ts, W, groups, auto_reset=False)
    obs = outputs(r.e, OBS8)
    for s in range(25):
        flags = np.zeros(W, np.int32)
        for at, w in resets:
            if at == s:
                flags[w] = 1
        k = r.stream_step(rec["acts"][s], resets=flags)
        r.check_after_direct(k, rec[s], obs, f"step {s}")
    r.close()
