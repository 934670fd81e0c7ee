"""The league scheduler without a GPU (include/mpenv_league.h, DESIGN.md §2
definition 20): mpenv_league_draw and mpenv_league_record -- the code k_league
runs (csrc/league_core.h) -- against the numpy restatement in league_testlib,
the buckets' edge cases, the layout, the host-side helpers of mpenv_league.py,
the header as C, and a sanitizer run of league_core.h in a stand-alone program."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import league_testlib as L
import mpenv_testlib as T

sys.path.insert(0, T.PKG)
import mpenv_league  # noqa: E402

CSRC = os.path.join(T.PKG, "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))


def random_weights(rng, P, kind):
    shape = (P + 1, P)
    if kind == 0:
        return np.zeros(shape, np.int32)                      # all-zero rows: no change
    if kind == 1:
        w = np.zeros(shape, np.int32)                         # a single non-zero entry per row
        w[np.arange(P + 1), rng.integers(0, P, P + 1)] = rng.integers(1, 100000, P + 1)
        return w
    if kind == 2:
        return rng.integers(-50, 50, shape).astype(np.int32)  # negative entries read as 0
    if kind == 3:
        return rng.integers(0, 200000, shape).astype(np.int32)  # entries above 65535 read as 65535
    if kind == 4:
        w = rng.integers(0, 20, shape).astype(np.int32)       # some rows zero, some not
        w[rng.integers(0, P + 1)] = 0
        return w
    return rng.integers(np.iinfo(np.int32).min, np.iinfo(np.int32).max, shape, dtype=np.int64).astype(np.int32)


def random_ids(rng, P, team):
    ids = np.repeat(rng.integers(-2, P + 3, (2, 1)), team, axis=1).astype(np.int32)
    for t in range(2):
        if team > 1 and rng.random() < 0.2:
            ids[t, rng.integers(1, team)] += 1                # a mixed team
    return ids


def test_draw_and_record_match_the_restatement():
    rng = np.random.default_rng(20)
    seen = dict(nochange=0, P1=0, P32=0, mixed=0)
    for k in range(2000):
        P = (1, 32)[k % 2] if k % 4 < 2 else int(rng.integers(1, 33))
        team = int(rng.integers(1, 7))
        mode = int(rng.integers(0, 3))
        seed, world, n = (int(v) for v in rng.integers(0, 2 ** 32, 3))
        n = n % 7 if k % 3 else n
        w = random_weights(rng, P, k % 6)
        ids = random_ids(rng, P, team)
        cfg = L.config(P, mode, seed)
        rc, got = L.draw(cfg, world, n, w, ids)
        assert rc == 0, L.err()
        want = L.ref_draw(P, mode, seed, world, n, w, ids)
        assert (got == want).all(), (k, P, mode, ids, got, want)
        if mode == L.TEAM1:
            assert (got[0] == ids[0]).all()
        seen["nochange"] += int(mode != L.NONE and (got == ids).all())
        seen["P1"] += P == 1
        seen["P32"] += P == 32
        seen["mixed"] += L.ref_team_id(ids[0]) == -1 and ids[0, 0] != -1
        # one episode on top of a random table
        mr = np.array([rng.integers(-1, 4), *rng.integers(0, 40, 4)], np.int32)
        table = rng.integers(0, 2 ** 40, (P + 1, P + 1, 8), dtype=np.int64)
        exp = table.copy()
        L.ref_record(P, mr, ids, exp)
        assert L.record(cfg, mr, ids, table) == 0, L.err()
        assert (table == exp).all(), (k, mr, ids)
    assert min(seen.values()) >= 50, seen


def test_null_weights_are_all_ones():
    ids = np.array([[0, 0], [1, 1]], np.int32)
    for n in range(20):
        cfg = L.config(5, L.BOTH, 77)
        rc, a = L.draw(cfg, 9, n, None, ids)
        rc2, b = L.draw(cfg, 9, n, np.ones((6, 5), np.int32), ids)
        assert rc == rc2 == 0 and (a == b).all()


def test_pick_is_proportional_to_the_clamped_weights():
    """Over 6,000 worlds' first draws the picks follow weights {0, 1, 3, 70000 -> 65535, -5 -> 0} scaled."""
    P = 5
    w = np.ones((P + 1, P), np.int32)
    w[0] = [0, 1, 3, 0, -5]
    cfg = L.config(P, L.TEAM1, 3)
    ids = np.array([[0], [4]], np.int32)
    counts = np.zeros(P, int)
    for world in range(6000):
        counts[L.draw(cfg, world, 0, w, ids)[1][1, 0]] += 1
    assert counts[0] == counts[3] == counts[4] == 0
    assert abs(counts[2] / 6000 - 0.75) < 0.03, counts  # 5 sigma of a binomial(6000, 0.75) is 0.028


def test_bucket_edge_cases():
    P = 4
    cfg = L.config(P, L.NONE)
    mr = np.array([0, 2, 1, 5, 6], np.int32)
    cases = [((-1, -1), P), ((P - 1, P - 1), P - 1), ((P, P), P), ((40, 40), P), ((1, 2), P), ((0, 0), 0)]
    for ids0, b0 in cases:
        for ids1, b1 in cases:
            table = np.zeros((P + 1, P + 1, 8), np.int64)
            assert L.record(cfg, mr, np.array([ids0, ids1], np.int32), table) == 0
            want = np.zeros_like(table)
            want[b0, b1] = [1, 1, 0, 0, 2, 1, 5, 6]
            assert (table == want).all(), (ids0, ids1)
    # the result column: 1 and 2 count as team 1's win and a draw, anything else in column 0 only
    for r, cols in ((1, [1, 0, 1, 0]), (2, [1, 0, 0, 1]), (-1, [1, 0, 0, 0]), (3, [1, 0, 0, 0])):
        table = np.zeros((P + 1, P + 1, 8), np.int64)
        assert L.record(cfg, np.array([r, 0, 0, 0, 0], np.int32), np.array([[1, 1], [2, 2]], np.int32), table) == 0
        assert list(table[1, 2, :4]) == cols and table.sum() == sum(cols)
    # row P serves every team that is no league policy; a mixed home team draws its opponent from it
    w = np.zeros((P + 1, P), np.int32)
    w[P, 3] = 1
    for ids0 in ((-1, -1), (P, P), (40, 40), (1, 2)):
        rc, got = L.draw(L.config(P, L.TEAM1, 1), 0, 0, w, np.array([ids0, (0, 0)], np.int32))
        assert rc == 0 and (got[0] == ids0).all() and (got[1] == 3).all()
    rc, got = L.draw(L.config(P, L.TEAM1, 1), 0, 0, w, np.array([(P - 1, P - 1), (0, 0)], np.int32))
    assert rc == 0 and (got[1] == 0).all()  # row P - 1 is all zero: no change


def test_layout_and_refusals():
    rc, t, w, d = L.layout(L.config(8), 16384)
    assert (rc, t, w, d) == (0, 9 * 9 * 8 * 8, 9 * 8 * 4, 16384 * 4)
    assert L.layout(L.config(1), 1)[1:] == (4 * 8 * 8, 2 * 4, 4)
    assert L.layout(L.config(32), 70)[1:] == (33 * 33 * 64, 33 * 32 * 4, 280)
    for cfg, needle in ((L.config(0), "num_policies"), (L.config(33), "num_policies"), (L.config(-1), "num_policies"),
                        (L.config(3, 3), "draw"), (L.config(3, -1), "draw")):
        assert L.layout(cfg, 4)[0] == L.ERR_INVALID and needle in L.err()
        assert L.draw(cfg, 0, 0, None, np.zeros((2, 1), np.int32))[0] == L.ERR_INVALID and needle in L.err()
    assert L.layout(L.config(3), 0)[0] == L.ERR_INVALID and "num_worlds" in L.err()
    assert L.draw(L.config(3), 0, 0, None, np.zeros((2, 7), np.int32))[0] == L.ERR_INVALID and "team_size" in L.err()
    # a null manager, and null outputs
    lib = L.lib()
    assert lib.mpenv_league_enable(None, C.byref(L.config(3))) == L.ERR_INVALID and "null" in L.err()
    for fn in ("mpenv_league_disable",):
        assert getattr(lib, fn)(None) == L.ERR_INVALID and "null" in L.err()
    assert lib.mpenv_league_clear(None, None) == L.ERR_INVALID and "null" in L.err()
    assert lib.mpenv_league_set_weights(None, None) == L.ERR_INVALID and "null" in L.err()
    assert lib.mpenv_league_enabled(None, None, None) == L.ERR_INVALID and "null" in L.err()
    assert lib.mpenv_league_tensor(None, 0, None, None, None, None, None) == L.ERR_INVALID and "null" in L.err()


def test_python_module_exposes_the_league():
    import madrona_mp_env as m

    for name in ("enable_league", "disable_league", "league_config", "league_table", "league_weights", "league_draws",
                 "clear_league", "set_league_weights"):
        assert hasattr(m.SimManager, name), name
    rng = np.random.default_rng(4)
    names = {L.NONE: "none", L.TEAM1: "team1", L.BOTH: "both"}
    for k in range(100):
        P, mode, team = int(rng.integers(1, 33)), int(rng.integers(0, 3)), int(rng.integers(1, 7))
        w = random_weights(rng, P, k % 6)
        ids = random_ids(rng, P, team)
        got = m.league_draw(P, names[mode], 11, 1000 + k, k % 4, ids, w)
        assert (np.asarray(got) == L.ref_draw(P, mode, 11, 1000 + k, k % 4, w, ids)).all()
        table = np.zeros((P + 1, P + 1, 8), np.int64)
        exp = table.copy()
        mr = np.array([k % 3, 1, 2, 3, 4], np.int32)
        L.ref_record(P, mr, ids, exp)
        out = m.league_record(P, mr, ids, table)
        assert (np.asarray(out) == exp).all() and (table == exp).all()
    with pytest.raises(Exception, match="num_policies"):
        m.league_draw(40, "team1", 0, 0, 0, np.zeros((2, 1), np.int32))
    with pytest.raises(Exception, match="draw"):
        m.league_draw(4, "sideways", 0, 0, 0, np.zeros((2, 1), np.int32))


# ------------------------------------------------------------ mpenv_league.py
def hand_table():
    """P = 2.  0 at home against 1: 10 episodes, 6 wins, 2 losses, 2 draws; 1 at home against 0:
    4 episodes, 1 win, 3 losses; 0 against 0: 2 draws; the external learner (bucket 2) at home
    against 1: 5 episodes, 5 wins.  1 against 1 never met."""
    t = np.zeros((3, 3, 8), np.int64)
    t[0, 1, :4] = [10, 6, 2, 2]
    t[1, 0, :4] = [4, 1, 3, 0]
    t[0, 0, :4] = [2, 0, 0, 2]
    t[2, 1, :4] = [5, 5, 0, 0]
    return t


def test_win_rates():
    wr = mpenv_league.win_rates(hand_table())
    assert wr.shape == (3, 3)
    assert wr[0, 1] == 0.7 and wr[1, 0] == 0.25 and wr[0, 0] == 0.5 and wr[2, 1] == 1.0
    assert np.isnan(wr[1, 1]) and np.isnan(wr[2, 2]) and np.isnan(wr[1, 2])
    # an episode with another result code counts as played, not as decided
    t = hand_table()
    t[1, 1, 0] = 3
    assert np.isnan(mpenv_league.win_rates(t)[1, 1])
    with pytest.raises(ValueError):
        mpenv_league.win_rates(np.zeros((3, 2, 8)))


def test_pfsp_weights():
    t = hand_table()
    # 0 against 1 over both seatings: wins 6 + 3 = 9, losses 2 + 1 = 3, draws 2: (9 + 1) / 14
    sym = mpenv_league.symmetric_win_rates(t)
    assert abs(sym[0, 1] - 10 / 14) < 1e-15 and abs(sym[1, 0] - 4 / 14) < 1e-15 and sym[0, 0] == 0.5
    w = mpenv_league.pfsp_weights(t, power=1.0)
    assert w.shape == (3, 2) and w.dtype == np.int32
    # row 0: priorities 0.5 (itself) and 4/14: the larger scales to 65535
    assert list(w[0]) == [65535, int(np.rint(4 / 14 / 0.5 * 65535))]
    # row 1: 10/14 against 0, 0.5 against itself (never met)
    assert list(w[1]) == [65535, int(np.rint(0.5 / (10 / 14) * 65535))]
    # row 2 (the external learner): 0.5 against 0 (never met); it always beat 1: priority 0, weight 0
    assert list(w[2]) == [65535, 0]
    # power 0: every opponent alike, 0 ** 0 included
    assert (mpenv_league.pfsp_weights(t, power=0.0) == 65535).all()
    # home rows only; a smaller scale; weights stay >= 1 where the priority is positive
    w = mpenv_league.pfsp_weights(t, home=2, power=2.0, scale=100)
    assert (w[:2] == 1).all() and list(w[2]) == [100, 0]
    t[2, 0, :4] = [1000, 999, 1, 0]
    w = mpenv_league.pfsp_weights(t, home=[2], power=3.0, scale=10)
    assert list(w[2]) == [10, 0]
    t[2, 1, :4] = [1000, 500, 500, 0]
    assert list(mpenv_league.pfsp_weights(t, home=[2], power=3.0, scale=10)[2]) == [1, 10]
    # a row that beats everyone every time is uniform
    t[2, 0, :4], t[2, 1, :4] = [5, 5, 0, 0], [5, 5, 0, 0]
    assert list(mpenv_league.pfsp_weights(t, home=[2])[2]) == [65535, 65535]
    assert mpenv_league.pfsp_weights(t).max() <= L.MAX_WEIGHT
    with pytest.raises(ValueError):
        mpenv_league.pfsp_weights(t, scale=65536)


# ------------------------------------------------------------ the header and the core
def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "league_c.c"
    src.write_text('#include "mpenv.h"\n'
                   "int use(mpenv_manager *m) {\n"
                   "    mpenv_league_config c = { 8, MPENV_LEAGUE_DRAW_TEAM1, 1u, 0 };\n"
                   "    int64_t t, w, d;\n"
                   "    int32_t ids[4] = { 0, 0, 1, 1 }, mr[5] = { 0, 1, 2, 3, 4 };\n"
                   "    int64_t table[9 * 9 * MPENV_LEAGUE_COLUMNS] = { 0 };\n"
                   "    return mpenv_league_enable(m, &c) + mpenv_league_layout(&c, 4, &t, &w, &d) +\n"
                   "           mpenv_league_draw(&c, 0, 0, 0, 2, ids) + mpenv_league_record(&c, mr, ids, 2, table) +\n"
                   "           mpenv_league_clear(m, 0) + MPENV_LEAGUE_TABLE + MPENV_LEAGUE_WEIGHTS + MPENV_LEAGUE_DRAWS +\n"
                   "           MPENV_LEAGUE_DRAW_NONE + MPENV_LEAGUE_DRAW_BOTH + MPENV_DTYPE_INT64;\n"
                   "}\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(T.ROOT, "include"), "-c",
                    str(src), "-o", str(tmp_path / "league_c.o")], check=True)


def test_core_under_address_and_undefined_sanitizers(tmp_path):
    """league_core.h's host functions in a stand-alone program (tests/league_host.cpp, its own main)
    built with -fsanitize=address,undefined and run directly; nothing of it is loaded into Python."""
    exe = tmp_path / "league_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(HERE, "league_host.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
