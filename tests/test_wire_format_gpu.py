"""The learner exchange's wire kernels (csrc/wire.hip) against
tests/wire_ref.py, the NumPy statement of wire format version 1, and at
shapes where no count divides evenly.

tests/test_wire_gpu.py checks unpack(pack(x)) == x at 6v6 x 16384, 6v6 x 512
and 3v3 x 64, where A * 80 is a multiple of 1024 and W is even.  A round trip
cannot see a mistake both kernels make the same way, nor a pack kernel that
writes outside its columns.  Here:
  * the pack kernel's message is compared with wire_ref.encode byte for byte,
    every byte the format does not define still holding the buffer's fill,
    and the unpack kernel's outputs with wire_ref.decode, at 1v1 x 3, 3v3 x 5,
    5v5 x 15 and 6v6 x 7: a partial last 1024-ray block (unpack), a partial
    last wave (pack: A * 80 % 64 == 32 when A % 4 == 2), odd W (the partial
    16-B piece of the [W][30] match copy, both kernels);
  * a 420-step round trip at 1v1 x 3 and 3v3 x 5 in which an episode ends by
    itself, agents die and respawn, and worlds are reset before the first
    plain message, in consecutive messages, right after a keyframe and in a
    keyframe's own step;
  * the pack kernel's own refusals: a value outside the packed word's bytes,
    a lidar ray off the (t, one-hot) / (-1, 0, 0, 0) pattern.

Bits of the last plane word beyond A * 80 cannot be set by these shapes:
A * 80 is a multiple of 32 for every legal A (A is even), so the last word is
always whole.  What the shapes exercise is the partial *wave* of the pack
kernel's ballots, not a partial word."""
import ctypes as C

import numpy as np
import pytest

import mpenv_testlib as T
import wire_ref as R

pytestmark = pytest.mark.gpu

REFUSED, DESYNC = 1, 2
FILL = 0xA5
GUARD = 512
EP_COL = 11  # MPENV_DBG_WI_EPISODE_COUNTER
NP_DTYPES = {0: np.int32, 1: np.float32, 2: np.uint32, 3: np.uint8, 4: np.uint16, 5: np.uint64}


def download(e, ptr, n):
    out = np.empty(n, np.uint8)
    e.mem.d2h(ptr, n, out)
    return out


def train_outputs(e):
    e.mem.hip.hipDeviceSynchronize()
    return {n: e.get(ex) for n, ex in T.TRAIN_OUTPUTS.items()}


def compare_outputs(sh, e, where):
    got, want = train_outputs(sh), train_outputs(e)
    for n in T.TRAIN_OUTPUTS:
        T.compare(got[n], want[n], f"{n} (shadow vs sender) @ {where}")


class Snapshot:
    """A state snapshot (mpenv_state_save) on the host, its sections by name
    (mpenv_state_section)."""

    def __init__(self, e):
        lib = T.lib_mpenv()
        self.e, self.nbytes = e, e.state_bytes()
        self.dev = e.mem.upload(np.full(self.nbytes, FILL, np.uint8))
        e.state_save(self.dev)
        e.mem.hip.hipDeviceSynchronize()
        self.host = download(e, self.dev, self.nbytes)
        dims = T.state_dims(e)
        self.sections = {}
        k = 0
        while True:
            sec, dt = T.state_section(k, *dims), C.c_int32()
            if sec is None:
                break
            assert lib.mpenv_state_section_dtype(k, C.byref(dt)) == 0
            self.sections[sec["name"]] = (sec["offset"], sec["bytes"], NP_DTYPES[dt.value])
            k += 1

    def column(self, name, host=None):
        off, nb, dt = self.sections[name]
        return (self.host if host is None else host)[off:off + nb].view(dt)

    def load(self, host=None):
        """restore the engine from this snapshot, or from an edited copy of its bytes"""
        if host is not None:
            self.e.mem.h2d(self.dev, host)
        self.e.state_load(self.dev)
        self.e.mem.hip.hipDeviceSynchronize()
        if host is not None:
            self.e.mem.h2d(self.dev, self.host)
        assert self.e.state_error() == 0

    def free(self):
        self.e.mem.free(self.dev)


def sender_after_combat(ts, W, steps=40, **kw):
    e = T.Engine(W, ts, sim_flags=1, **kw)
    e.put_ctrl([0, 1, 1])
    e.init()
    for s in range(steps):
        e.set_actions(T.combat_actions(e, s))
        e.step()
    return e


def wire_columns(e, snap, keyframe, host=None):
    """The message's columns as wire_ref.encode takes them: internal state by
    name from a snapshot (or an edited copy of its bytes), exports from
    Engine.get."""
    A = e.W * e.N
    cols = {n: snap.column(n, host) for n in R.AF + R.AI + R.WI + R.PACKED + ("visMask",)}
    for name, ex in (("hp", "HP"), ("alive", "ALIVE"), ("reward", "REWARD"), ("done", "DONE"),
                     ("magazine", "MAGAZINE"), ("rewardCoefs", "REWARD_HYPER_PARAMS"),
                     ("matchResult", "MATCH_RESULT")):
        cols[name] = e.get(ex)
    cols["lidar"] = np.concatenate([e.get("FWD_LIDAR").reshape(A, R.FWD_RAYS, 4),
                                    e.get("REAR_LIDAR").reshape(A, R.REAR_RAYS, 4)], axis=1)
    if keyframe:
        cols["lkObs"] = e.get("OPPONENT_LAST_KNOWN_OBSERVATIONS")
        cols["lkPos"] = e.get("OPPONENT_LAST_KNOWN_POSITIONS")
    return cols


# ------------------------------------------------- D: each kernel against NumPy

def check_packed_bytes(e, snap, keyframe, world_offset, host=None):
    """Pack into a buffer of FILL, GUARD bytes longer than the message: every
    byte the format defines equals wire_ref.encode's, every other byte --
    column padding, the header's reserved words and the rest of its 256-B
    block, the guard -- is still FILL.  Returns (device buffer, message)."""
    A, W, N = e.W * e.N, e.W, e.N
    what = "keyframe" if keyframe else "plain"
    n = e.wire_bytes(keyframe)
    L = R.layout(A, W, keyframe)
    assert n == L["total"]
    buf = e.mem.upload(np.full(n + GUARD, FILL, np.uint8))
    e.wire_pack(buf, keyframe)
    msg = download(e, buf, n + GUARD)
    header = R.make_header(A, W, N, N // 2, keyframe, world_offset=world_offset)
    want, mask = R.encode(wire_columns(e, snap, keyframe, host), header)
    mask = np.concatenate([mask, np.zeros(GUARD, np.uint8)]).astype(bool)
    want = np.concatenate([want, np.zeros(GUARD, np.uint8)])
    for name, (off, nbytes, _, _) in [("header", (0, 48, None, None))] + R.column_items(L):
        bad = np.flatnonzero(msg[off:off + nbytes] != want[off:off + nbytes])
        assert bad.size == 0, (f"column {name} ({what}): {bad.size} bytes differ, first at +{bad[0]}: "
                               f"packed 0x{msg[off + bad[0]]:02x}, format 0x{want[off + bad[0]]:02x}")
    assert (msg[mask] == want[mask]).all()
    stray = np.flatnonzero(msg[~mask] != FILL)
    assert stray.size == 0, (f"{what}: {stray.size} bytes outside the format's columns were written, first at "
                             f"{np.flatnonzero(~mask)[stray[0]]} of {n} (+{GUARD} guard)")
    return buf, msg[:n], header


# (team size, worlds, world_id_offset, lidar classes in the message): the classes
# are what the CPU oracle's lidar holds after these 40 steps (seed 5) -- rays
# that hit nothing (class 0, the kernel's initial value) only at 5v5 x 15, and
# nothing but walls at 1v1 x 3
D_SHAPES = [(1, 3, 0, {1}), (3, 5, 64, {1, 2, 3}), (5, 15, 0, {0, 1, 2, 3}), (6, 7, 0, {1, 2, 3})]


@pytest.mark.parametrize("ts,W,world_offset,classes", D_SHAPES, ids=[f"{t}v{t}x{w}" for t, w, _, _ in D_SHAPES])
def test_pack_and_unpack_against_the_numpy_format(ts, W, world_offset, classes):
    N = 2 * ts
    A = W * N
    # what the shape exercises, from the shape
    if ts in (1, 3, 5):
        assert A * R.RAYS % 64 == 32      # pack: a partial last wave of rays
    assert A * R.RAYS % 1024 != 0         # unpack: a partial last 1024-ray block
    assert A * R.RAYS % 32 == 0           # never a partial plane word (module docstring)
    assert W * 30 * 4 % 16 == 8           # the match copy's partial 16-B piece

    e = sender_after_combat(ts, W, world_id_offset=world_offset)
    sh = T.Engine(W, ts, sim_flags=1, world_id_offset=world_offset)
    rng = np.random.default_rng(7)
    e.put("MATCH_RESULT", rng.integers(-5, 1000, (W, 30)))  # every byte of the match copy tells
    snap = Snapshot(e)
    lidar_seen = set()
    for keyframe in (True, False):  # the shadow needs the keyframe first
        buf, msg, header = check_packed_bytes(e, snap, keyframe, world_offset)

        # the unpack kernel by itself: outputs that are message columns, every byte pre-filled
        for ex in ("FWD_LIDAR", "REAR_LIDAR", "HP", "ALIVE", "REWARD", "MAGAZINE", "REWARD_HYPER_PARAMS", "DONE",
                   "MATCH_RESULT"):
            sh.put(ex, np.full(sh.desc(ex)[2], 7))
        sh.wire_unpack(buf, keyframe)
        assert sh.wire_error() == 0
        hdr, cols = R.decode(msg)
        assert hdr == header
        got_lidar = np.concatenate([sh.get("FWD_LIDAR").reshape(A, R.FWD_RAYS, 4),
                                    sh.get("REAR_LIDAR").reshape(A, R.REAR_RAYS, 4)], axis=1)
        T.compare(got_lidar, cols["lidar"], "lidar (shadow vs decode)")
        for name, ex in (("hp", "HP"), ("alive", "ALIVE"), ("reward", "REWARD"), ("done", "DONE"),
                         ("magazine", "MAGAZINE"), ("rewardCoefs", "REWARD_HYPER_PARAMS"),
                         ("matchResult", "MATCH_RESULT")):
            g = sh.get(ex)
            T.compare(g, cols[name].reshape(g.shape).astype(g.dtype), f"{ex} (shadow vs decode)")
        if keyframe:
            T.compare(sh.get("OPPONENT_LAST_KNOWN_OBSERVATIONS"), cols["lkObs"], "last-known rows (shadow vs decode)")
            T.compare(sh.get("OPPONENT_LAST_KNOWN_POSITIONS"), cols["lkPos"], "last-known positions (shadow vs decode)")
        compare_outputs(sh, e, "keyframe" if keyframe else "plain")
        hot = cols["lidar"][..., 1:]
        lidar_seen |= set(int(c) for c in np.unique(np.where(hot.any(-1), hot.argmax(-1) + 1, 0)))
        e.mem.free(buf)
    assert lidar_seen == classes, lidar_seen
    # the packed word with all four bytes in use (the rollout's poses and
    # weapon are 0 at this step, so only the flags byte was): any values the
    # bytes can hold, through a snapshot load; packed only
    host = snap.host.copy()
    for name in R.PACKED:
        snap.column(name, host)[:] = rng.integers(0, 256, A)
    snap.load(host)
    buf, msg, _ = check_packed_bytes(e, snap, False, world_offset, host)
    assert msg[8:12].view(np.uint32)[0] == 0  # in range: no overflow flag
    e.mem.free(buf)
    snap.load()
    snap.free()
    e.close()
    sh.close()


# ----------------------------------- E: round trip with every episode-counter move

@pytest.mark.parametrize("ts,W", [(1, 3), (3, 5)])
def test_round_trip_at_ragged_shapes_with_every_episode_counter_move(ts, W):
    """Sender: seed 5, sim_flags 1, the aim-bot on its own observations, HP set
    to 1 for everyone at step 20 (deaths and respawns follow).  On the CPU
    oracle, which the engine equals bit for bit, world 0 starts at curStep
    2602 and its episode ends by itself at step 397 (counter 1 -> 2), and
    respawnSteps > 0 shows on 5 agent-steps at 1v1 x 3 and 19 at 3v3 x 5."""
    steps = 420
    ragged = (ts, W) == (3, 5)
    e = T.Engine(W, ts, sim_flags=1)
    sh = T.Engine(W, ts, sim_flags=1)    # fed from a keyframe at init, then a plain message every step
    late = T.Engine(W, ts, sim_flags=1)  # joins by keyframe at step 100
    e.put_ctrl([0, 1, 1])
    e.init()
    buf = e.mem.upload(np.zeros(e.wire_bytes(True), np.uint8))
    e.wire_pack(buf, True)
    sh.wire_unpack(buf, True)
    assert sh.wire_error() == 0
    compare_outputs(sh, e, "init")
    e.enable_stats(True)
    # triggered resets: {step: world}, before that step
    triggers = {}
    if ragged:
        triggers = {0: 1,            # before the first plain message
                    50: 2, 51: 2,    # the same world in consecutive messages
                    101: 3,          # the first plain message after `late`'s keyframe
                    150: 1}          # in the step whose message goes to `late` as a keyframe
    ep = [e.get("DEBUG_WORLD_I32")[:, EP_COL].copy()]
    respawning = 0
    for s in range(steps):
        if s in triggers:
            e.trigger_reset(triggers[s])
        if s == 20:
            e.put("HP", np.ones(W * 2 * ts, np.float32))
        e.set_actions(T.combat_actions(e, s))
        e.step()
        e.wire_pack(buf, False)
        sh.wire_unpack(buf, False)
        compare_outputs(sh, e, f"step {s}")
        if s > 100 and not (ragged and s == 150):
            late.wire_unpack(buf, False)
        if s == 100 or (ragged and s == 150):
            e.wire_pack(buf, True)
            late.wire_unpack(buf, True)
        if s >= 100:
            compare_outputs(late, e, f"step {s} (keyframe at 100)")
        ep.append(e.get("DEBUG_WORLD_I32")[:, EP_COL].copy())
        respawning += int((e.get("DEBUG_AGENT_I32")[:, 7] > 0).sum())
    assert sh.wire_error() == 0 and late.wire_error() == 0
    ep = np.stack(ep)  # [steps + 1, W]
    # an episode counter moved by itself: in a world, at a step, without a triggered reset
    moved = [(s, w) for s in range(steps) for w in range(W) if ep[s + 1, w] != ep[s, w]]
    own = [(s, w) for s, w in moved if triggers.get(s) != w]
    assert own, moved
    assert (397, 0) in own, own
    if ragged:  # and every triggered reset moved its world's counter in its own step
        assert all((s, w) in moved for s, w in triggers.items()), (moved, triggers)
    assert respawning > 0
    assert e.read_stats()["kills"] > 0
    assert (e.get("OPPONENT_LAST_KNOWN_OBSERVATIONS") != 0).any()
    assert (e.get("OPPONENT_LAST_KNOWN_POSITIONS") != 0).any()
    e.mem.free(buf)
    for x in (e, sh, late):
        x.close()


# -------------------------------------------- F: the pack kernel's own refusals

def test_pack_flags_values_the_format_cannot_carry():
    ts, W = 3, 5
    A = W * 2 * ts
    e = sender_after_combat(ts, W)
    sh = T.Engine(W, ts, sim_flags=1)
    snap = Snapshot(e)
    buf = e.mem.upload(np.full(e.wire_bytes(True), FILL, np.uint8))

    def resync(where):
        e.wire_pack(buf, True)
        assert download(e, buf, 12)[8:12].view(np.uint32)[0] == R.FLAG_KEYFRAME, where
        sh.wire_unpack(buf, True)
        assert sh.wire_error() == 0, where
        compare_outputs(sh, e, where)

    def weapon_256():
        host = snap.host.copy()
        snap.column("weapon", host)[A - 1] = 256
        snap.load(host)

    def cur_pose_minus_1():
        host = snap.host.copy()
        snap.column("curPose", host)[0] = -1
        snap.load(host)

    def lidar_off_pattern():
        fwd = e.get("FWD_LIDAR")
        fwd.reshape(A, R.FWD_RAYS, 4)[A - 1, 37] = (0.5, 1, 1, 0)
        e.put("FWD_LIDAR", fwd)

    resync("before the refusals")
    for corrupt in (weapon_256, cur_pose_minus_1, lidar_off_pattern):
        for keyframe in (False, True):
            corrupt()
            before = train_outputs(sh)
            e.wire_pack(buf, keyframe)
            flags = int(download(e, buf, 12)[8:12].view(np.uint32)[0])
            assert flags == R.FLAG_OVERFLOW | (R.FLAG_KEYFRAME if keyframe else 0), (corrupt.__name__, keyframe, flags)
            sh.wire_unpack(buf, keyframe)
            assert sh.wire_error() == REFUSED | DESYNC, (corrupt.__name__, keyframe)
            after = train_outputs(sh)
            for n in T.TRAIN_OUTPUTS:
                assert before[n].tobytes() == after[n].tobytes(), (corrupt.__name__, keyframe, n)
            # the sender restored: its next keyframe is accepted and the shadow equals it
            snap.load()
            resync(f"after {corrupt.__name__} ({'keyframe' if keyframe else 'plain'})")
    assert sh.wire_error() == 0
    e.mem.free(buf)
    snap.free()
    e.close()
    sh.close()
