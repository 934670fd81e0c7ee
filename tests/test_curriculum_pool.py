"""The live curriculum pool without a GPU (include/mpenv_curriculum.h, DESIGN.md
§2 definition 21): the host entry points of csrc/curriculum_core.h -- layout,
selection and packing -- against the numpy restatement of
tests/curriculum_testlib.py, their refusals, and mpenv_curriculum.py's files."""
import os
import subprocess

import numpy as np
import pytest

import curriculum_testlib as CT
import mpenv_testlib as T

MC = CT.MC


def test_layout_sizes():
    for cap, R in ((1, 1), (5, 1), (64, 2), (4096, 32)):
        rc, pool, ticks = CT.layout(CT.config(cap), R)
        assert rc == 0, CT.err()
        assert pool == R * cap * 176 and ticks == R * cap * 4
        assert pool % 16 == 0
    assert MC.SNAPSHOT.itemsize == 176 and MC.SNAPSHOT == T.CURRICULUM_SNAPSHOT


@pytest.mark.parametrize("first,n", [(0, 16), (5, 3), (0, 1)])
def test_select_matches_restatement(first, n):
    seed, offset = 11, 7
    slots = np.arange(64)
    for r in (0, 1):
        for period in (0, 1, 2, 7):
            hits = 0
            for t in range(1, 33):
                ref, world = CT.ref_select(seed, offset, slots, t, period, first, n)
                got = [CT.select(seed, offset, r, int(s), t, period, first, n) for s in slots]
                assert all(g[0] == 0 for g in got), CT.err()
                np.testing.assert_array_equal([g[1] for g in got], ref.astype(int), err_msg=f"refresh r{r} p{period} t{t}")
                np.testing.assert_array_equal([g[2] for g in got], world, err_msg=f"world r{r} p{period} t{t}")
                assert all(first <= g[2] < first + n for g in got)
                hits += int(ref.sum())
            if period == 1:
                assert hits == 64 * 32
            elif period == 0:
                assert hits == 0
            else:  # about 1 / period of 2048 draws
                assert 0.5 * 2048 / period < hits < 1.5 * 2048 / period
    # the value depends on the seed, the range's first global world, the slot (the rows differ) and the tick
    base = CT.ref_hash(seed, offset + first, slots, 3)
    assert len(set(base[0].tolist())) == 64
    for other in (CT.ref_hash(seed + 1, offset + first, slots, 3), CT.ref_hash(seed, offset + first + 1, slots, 3),
                  CT.ref_hash(seed, offset + first, slots, 4)):
        assert not np.array_equal(base[0], other[0]) and not np.array_equal(base[1], other[1])
    # a range is its first world's global id: range 1 at offset 0 draws as range 0 of a manager at that offset
    assert CT.select(seed, 0, 1, 5, 9, 2, 8, n)[1:] == tuple(
        np.array(CT.select(seed, 8, 0, 5, 9, 2, 0, n)[1:]) + (0, 8))
    assert CT.select(seed, 0, 32, 5, 9, 2, 8, n)[0] == CT.ERR_INVALID and "range" in CT.err()


def hand_rows(team_size):
    """Hand-made worlds: yaw exactly +pi (wraps to -32768), negative positions, hp 0, crouch and prone,
    a zone that is not captured, a world just reset."""
    n = 2 * team_size
    k = np.arange(n)
    pos = np.stack([-300.5 + 77.25 * k, 120.75 - 41.5 * k, 0.9 + 3.3 * k], 1)
    yaw = np.linspace(-np.pi, np.pi, n).astype(np.float32)
    yaw[-1] = CT.PI  # exactly +pi
    yaw[0] = -CT.PI
    pitch = np.linspace(-0.25 * np.pi, 0.25 * np.pi, n).astype(np.float32)
    hp = np.array([0, 100, 37.9, 0.4, 99.99, 1][:n] * 2, np.float32)[:n]
    mag = np.stack([(30 - 3 * k) % 31, k % 3], 1)
    pose = k % 3
    landed = np.where(k % 4 == 1, (k + 1) % n, -1)
    a = CT.world_rows(1234, 2, 1, 1, 600, 17, pos, yaw, pitch, hp, mag, pose, landed)
    b = CT.world_rows(1, 0, 0, 1, 333, 20, pos[::-1], yaw[::-1], pitch, hp[::-1], mag, pose[::-1], landed)  # not captured
    c = CT.world_rows(0, 1, 1, 0, 1, 0, -pos, yaw, -pitch, hp, mag, pose, landed)  # a world just reset: step 0
    return [a, b, c]


@pytest.mark.parametrize("team_size", [6, 3, 1])
def test_pack_matches_restatement(team_size):
    n = 2 * team_size
    for rows in hand_rows(team_size):
        rc, got = CT.pack(rows, team_size)
        assert rc == 0, CT.err()
        want = CT.ref_pack(rows, team_size)
        assert got.tobytes() == want.tobytes(), (got, want)
        assert got["players"][n:].tobytes() == bytes(14 * (12 - n))  # players >= N are zero
    rc, a = CT.pack(hand_rows(team_size)[0], team_size)
    assert a["step"] == 1233 and a["controller"] == 1
    assert a["players"]["yaw"][n - 1] == -32768 and a["players"]["yaw"][0] == -32768  # +pi wraps onto -pi
    assert a["players"]["hp"][0] == 0 and a["players"]["pos"][0, 0] == -300
    if team_size >= 2:
        assert a["players"]["flags"][1] == 2 | 4 and a["players"]["flags"][2] == 8
    rc, b = CT.pack(hand_rows(team_size)[1], team_size)
    assert b["controller"] == -1 and b["step"] == 0
    rc, c = CT.pack(hand_rows(team_size)[2], team_size)
    assert c["step"] == 0 and c["controller"] == 0


def test_host_entry_points_refuse_bad_parameters():
    L = CT.lib()
    for cfg, word in ((CT.config(0), "capacity"), (CT.config(-3), "capacity"), (CT.config(4, period=-1), "period"),
                      (CT.config(4, step_range=(10, 9)), "step_lo"), (CT.config(4, need=8), "need")):
        rc, _, _ = CT.layout(cfg, 1)
        assert rc == CT.ERR_INVALID and word in CT.err(), CT.err()
    for R in (0, 33):
        assert CT.layout(CT.config(4), R)[0] == CT.ERR_INVALID and "num_ranges" in CT.err()
    assert L.mpenv_curriculum_pool_layout(None, 1, None, None) == CT.ERR_INVALID
    assert CT.select(0, 0, 0, 0, 1, -1, 0, 4)[0] == CT.ERR_INVALID and "period" in CT.err()
    assert CT.select(0, 0, 0, 0, 1, 1, 0, 0)[0] == CT.ERR_INVALID and "num_worlds" in CT.err()
    assert CT.select(0, 0, 0, 0, 1, 1, -1, 4)[0] == CT.ERR_INVALID
    assert L.mpenv_curriculum_pool_select(0, 0, 0, 0, 1, 1, 0, 4, None, None) == CT.ERR_INVALID
    rows = hand_rows(3)[0]
    assert CT.pack(rows, 0)[0] == CT.ERR_INVALID and "team_size" in CT.err()
    assert CT.pack(rows, 7)[0] == CT.ERR_INVALID
    assert L.mpenv_curriculum_pool_pack(None, 3, None) == CT.ERR_INVALID
    # the manager calls without a manager
    assert L.mpenv_curriculum_pool_enable(None, None) == CT.ERR_INVALID
    assert L.mpenv_curriculum_pool_disable(None) == CT.ERR_INVALID


def test_header_is_c(tmp_path):
    """mpenv_curriculum.h through mpenv.h as strict C11, every entry point and constant named"""
    src = tmp_path / "pool_c.c"
    src.write_text("#include \"mpenv.h\"\n"
                   "int use(mpenv_manager *m) {\n"
                   "    mpenv_curriculum_pool_config c = { 8, 64, 0, 2999, MPENV_CURRICULUM_NEED_CAPTURED |\n"
                   "        MPENV_CURRICULUM_NEED_CONTESTED | MPENV_CURRICULUM_NEED_BOTH_ALIVE, 1 };\n"
                   "    mpenv_curriculum_snapshot s[1];\n"
                   "    mpenv_curriculum_world w = { 0 };\n"
                   "    int64_t a, b, dims[8]; int32_t on, r, world, dt, nd; uint32_t t; void *p;\n"
                   "    return mpenv_curriculum_pool_enable(m, &c) + mpenv_curriculum_pool_configure(m, &c) +\n"
                   "           mpenv_curriculum_pool_enabled(m, &c, &on) + mpenv_curriculum_pool_tick(m, &t) +\n"
                   "           mpenv_curriculum_pool_tensor(m, MPENV_CURRICULUM_POOL, &p, &dt, &nd, dims, 0) +\n"
                   "           mpenv_curriculum_pool_tensor(m, MPENV_CURRICULUM_TICKS, &p, &dt, &nd, dims, 0) +\n"
                   "           mpenv_curriculum_pool_set(m, 0, 0, 1, s) + mpenv_curriculum_pool_disable(m) +\n"
                   "           mpenv_curriculum_pool_layout(&c, 1, &a, &b) +\n"
                   "           mpenv_curriculum_pool_select(1, 0, 0, 0, 1, 64, 0, 4, &r, &world) +\n"
                   "           mpenv_curriculum_pool_pack(&w, 6, s) + (int)sizeof(s) - MPENV_CURRICULUM_SNAPSHOT_BYTES;\n"
                   "}\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(T.ROOT, "include"), "-c",
                    str(src), "-o", str(tmp_path / "pool_c.o")], check=True)


def test_files_round_trip_and_equal_the_curriculum_file(tmp_path):
    src = T.make_curriculum_file(str(tmp_path / "a.bin"), n=48)
    snaps = MC.from_file(src)
    assert snaps.dtype == MC.SNAPSHOT and len(snaps) == 48
    dst = str(tmp_path / "b.bin")
    assert MC.to_file(snaps, dst) == 48
    assert open(dst, "rb").read() == open(src, "rb").read()
    # a pool as the manager hands it out: uint8 [R, capacity, 176]
    raw = np.frombuffer(open(src, "rb").read(), np.uint8).reshape(2, 24, 176)
    assert MC.to_file(raw, dst) == 48
    assert open(dst, "rb").read() == open(src, "rb").read()
    np.testing.assert_array_equal(MC.from_file(dst), snaps)
    with pytest.raises(ValueError):
        MC.as_snapshots(np.zeros((3, 175), np.uint8))
    d = MC.describe(snaps)
    assert d["count"] == 48 and d["step"].sum() == 48 and d["controller"].sum() == 48
    assert d["zone"].sum() == 48 and d["living"].sum() == 48 and d["living"][12] == 48  # the file's hp is 1..100
    np.testing.assert_array_equal(d["controller"], [(snaps["controller"] == c).sum() for c in (-1, 0, 1)])
    dead = snaps.copy()
    dead["players"]["hp"][:, :6] = 0
    d = MC.describe(dead)
    assert d["living"][6] == 48 and d["living_team"][0, 0] == 48 and d["living_team"][1, 6] == 48
