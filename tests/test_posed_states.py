"""oracle_put_debug and the posed-state case families, on the CPU with the
oracle alone (tests/posed_testlib.py; DESIGN.md §7 "Posed states").

The first half checks the inverse of refreshDebug: an identity pose changes
nothing for 20 further steps, an edited column reads back edited and nothing
else moves.  The second half is the families' coverage: the GPU half
(tests/test_posed_states_gpu.py) compares the engine with the oracle on these
cases, and a case that never reaches its branch would pass there vacuously --
so each branch is shown here, on the oracle's own outputs and a float64
restatement of the navmesh lookup.  Conditions, not tolerances."""
import functools

import numpy as np
import pytest

import mpenv_testlib as T
import posed_testlib as P

ALL = T.STEP_OUTPUTS + T.DEBUG_OUTPUTS + ["DEBUG_EXPLORE"]


def _twins(flags, steps, ts=3, W=5):
    a, b = T.Oracle(W, ts, sim_flags=flags), T.Oracle(W, ts, sim_flags=flags)
    for o in (a, b):
        o.put_ctrl([0, 1, 1])
        o.init()
    for s in range(steps):
        acts = T.seek_combat_actions(a, s)
        for o in (a, b):
            o.set_actions(acts)
            o.step()
    return a, b


def _same(a, b, where):
    for n in ALL:
        T.compare(a.get(n), b.get(n), f"{n} @ {where}")


@pytest.mark.parametrize("flags,at", [(1, 0), (1, 7), (1, 40), (1 | (1 << 11), 40), (0, 25)],
                         ids=["step0", "step7", "step40", "subzones_step40", "crumbs_step25"])
def test_identity_pose_changes_nothing(flags, at):
    """put_debug() with unedited arrays: bit-identical to an untouched twin for 20 further steps."""
    a, b = _twins(flags, at)
    if at == 25:
        assert a.get("DEBUG_WORLD_I32")[:, 15].max() > 0, "no crumbs at this step"
    if flags & (1 << 11):
        assert (a.get("DEBUG_WORLD_I32")[:, 21] != 0x11111111).any(), "no sub-zone state to carry"
    a.lib.oracle_refresh_debug(a.h)
    a.put_debug()
    _same(a, b, "after the identity pose")
    for s in range(at, at + 20):
        acts = T.seek_combat_actions(b, s)
        for o in (a, b):
            o.set_actions(acts)
            o.step()
        _same(a, b, f"step {s}")
    a.close()
    b.close()


def test_edited_pose_round_trip():
    """Every debug column in turn: the edit reads back, every other column and export is unchanged."""
    a, b = _twins(1 | (1 << 11), 12)
    before = {n: b.get(n) for n in ALL}
    rng = np.random.default_rng(3)
    for name, (exp, col) in P.COLUMNS.items():
        shape = before[exp][:, col].shape
        if exp.endswith("F32"):
            vals = rng.uniform(-500, 500, shape).astype(np.float32)
        elif name == "flags":
            vals = rng.integers(0, 64, shape).astype(np.int32)
        elif name == "visMask":
            vals = rng.integers(0, 8, shape).astype(np.int32)
        elif name == "numCrumbs":
            continue  # with the crumb rows, below
        elif name in ("finished", "contested", "captured", "earned"):
            vals = rng.integers(0, 2, shape).astype(np.int32)  # booleans in the oracle
        elif name == "subState":
            # a nibble per sub-zone: controller + 1 in {0, 1, 2}, contested 4, captured 8
            nib = rng.integers(0, 3, shape + (8,)) | (rng.integers(0, 4, shape + (8,)) << 2)
            vals = (nib << (4 * np.arange(8))).sum(-1).astype(np.uint32).view(np.int32)
        else:
            vals = rng.integers(-1, 1000, shape).astype(np.int32)
        P.pose(None, a, {name: (slice(None), vals)})
        for n in ALL:
            want = before[n].copy()
            if n == exp:
                want[:, col] = vals
            T.compare(a.get(n), want, f"{n} after editing {name}")
        P.pose(None, a, {name: (slice(None), before[exp][:, col])})
    # the crumb list with its length
    c = np.zeros_like(before["DEBUG_CRUMBS"])
    c[:, :100, :7] = rng.integers(0, 50, (a.W, 100, 7)).astype(np.float32)
    c[:, :100, 7] = 1
    P.pose(None, a, {"crumbs": (slice(None), c), "numCrumbs": (slice(None), np.full(a.W, 100, np.int32))})
    for n in ALL:
        want = before[n].copy()
        if n == "DEBUG_CRUMBS":
            want = c
        if n == "DEBUG_WORLD_I32":
            want[:, 15] = 100
        T.compare(a.get(n), want, f"{n} after editing the crumbs")
    a.close()
    b.close()


# ------------------------------------------------------------------ coverage
@functools.lru_cache(maxsize=None)
def records(name):
    fam = {"bots": P.BOTS, "combat": P.COMBAT, "zone": P.zone_family(), "zone_noreset": P.zone_family(False),
           "move": P.MOVE, "crumbs": P.CRUMBS}[name]
    return P.run_family(fam)


def test_bot_cases_cover_the_navmesh_lookup():
    """Start triangle by containment and by the fallback; table entry -1, goal and hop.  The
    classification is the float64 restatement's, an approximation of the oracle's float32 lookup: it
    is only counted where it cannot flip -- containment for the centroid rounds' bots (strictly inside
    their triangle), the fallback for bots 50 units outside the mesh's bounding box (inside no
    triangle in any precision).  The hop kinds rest on the float64 goal triangle, itself a fallback
    result; test_bot_cases_cover_both_sides_of_dot_and_cross checks on the oracle's actions that the
    targets they imply are the oracle's."""
    found = set()
    for r in records("bots"):
        if r["name"].startswith("centroids"):
            for start, inside, hop, _ in r["info"]["cls"]:
                if inside:
                    found |= {"containment", hop}
        if r["name"].startswith("outside"):
            found |= {"fallback" for g, c in enumerate(r["info"]["cls"]) if g % 2 == 1 and not c[1]}
    assert found >= {"containment", "fallback", "none", "goal", "hop"}, found


def test_bot_cases_cover_both_sides_of_dot_and_cross():
    """No wall in these rounds, so move_amount is 2 where dot > 0.6 and 0 elsewhere; a bot that does
    not fire turns by 0 / 1 (cross.z < 0) or 4 / 3: aim -10 / -5 or 10 / 5.  In the centroid rounds
    the float64 target is checked against the oracle: a bot turned exactly toward it moves and one
    turned exactly away does not, wherever the target is not the bot's own position (triangle 136 is
    vertical: its centroid lies in triangle 16, whose next hop is 136 again).  The yaws a few ulps
    either side of the cone land on no known side after sinf, cosf and normalize; the exact threshold
    is test_bot_case_sits_exactly_on_the_dot_threshold's."""
    checked = 0
    for r in records("bots"):
        if r["info"]["kind"] != "nav":
            continue
        act = r["steps"][0]["PVP_DISCRETE_ACTION"]
        aim = r["steps"][0]["PVP_AIM_ACTION"].reshape(-1, 2)[:, 0]
        assert set(np.unique(act[:, 0])) == {0, 2}, r["name"]
        assert (aim < 0).any() and (aim > 0).any(), r["name"]
        if not r["name"].startswith("centroids"):
            continue
        pos = r["posed"]["DEBUG_AGENT_F32"][:, :2]
        for g, (_, inside, hop, tgt) in enumerate(r["info"]["cls"]):
            kind = P.YAW_TURNS[g % len(P.YAW_TURNS)]
            if kind not in ("toward", "away") or not inside or np.linalg.norm(tgt - pos[g]) < 1.0:
                continue
            assert act[g, 0] == (2 if kind == "toward" else 0), (r["name"], g, kind, hop)
            checked += 1
    assert checked >= 100, checked


def test_bot_case_sits_exactly_on_the_dot_threshold():
    """Three bots at one point, the dot product one float below 0.6f, on it and one above, where the
    float64 lookup says the target is the zone centre: exactly 0.6f does not move, the float above
    does."""
    r = [r for r in records("bots") if r["info"]["kind"] == "exact"][0]
    act = r["steps"][0]["PVP_DISCRETE_ACTION"]
    ex = r["info"]["exact"]
    triples = [g for g in ex if ex[g] == -1 and ex.get(g + 1) == 0 and ex.get(g + 2) == 1]
    assert triples
    assert all(act[g:g + 3, 0].tolist() == [0, 0, 2] for g in triples), [act[g:g + 3, 0].tolist() for g in triples]


def test_wall_cases_cover_every_branch_of_the_switch():
    r = [r for r in records("bots") if r["info"]["kind"] == "wall"][0]
    act = r["steps"][0]["PVP_DISCRETE_ACTION"]
    angle = {0: 2, 1: 3, 2: 3, 3: 4, 4: 4, 5: 5, 6: 5, 7: 6}
    seen, bounds = set(), set()
    for g, mean in r["info"]["mean"].items():
        if mean is None:
            assert act[g, 1] == 0, g
            seen.add(None)
            continue
        case = int(mean / 32 * 8)
        assert act[g, 1] == angle[case], (g, mean)
        assert act[g, 0] == (2 if case in (3, 4) else 1), (g, mean)
        seen.add(case)
        if mean in (4.0, 12.0, 20.0, 28.0):
            bounds.add(mean)
    assert seen == set(range(8)) | {None}
    assert bounds == {4.0, 12.0, 20.0, 28.0}


def test_bot_cases_hold_a_reload_suppressed_fire():
    n = 0
    for r in records("bots"):
        if "vis" not in r["info"]:
            continue
        fire = r["steps"][0]["PVP_DISCRETE_ACTION"][:, 2]
        vis, mag = r["info"]["vis"], r["info"]["mag"]
        assert (fire[(vis != 0) & (mag > 0)] == 1).all()
        assert (fire[(vis != 0) & (mag == 0)] == 0).all()
        n += int(((vis != 0) & (mag == 0)).sum())
    assert n > 0


def test_combat_cases_cover_kills_hits_respawn_and_heal():
    exact = double = mutual = respawn = heal = 0
    for r in records("combat"):
        hp0 = r["posed"]["HP"].reshape(-1)
        s1 = r["steps"][0]
        ai = s1["DEBUG_AGENT_I32"]
        killed = (ai[:, 9] & 2) != 0
        for w, c in r["info"]["worlds"].items():
            a, b = c["a"], c["b"]
            exact += int(killed[b] and hp0[b] == P.DMG and ai[b, 10] == 1)
            double += int(ai[b, 10] == 2)
            mutual += int(killed[a] and killed[b])
            # a killed agent respawns within its step: alive again at full hp, somewhere else
            moved = (s1["DEBUG_AGENT_F32"][b, :3] != r["posed"]["DEBUG_AGENT_F32"][b, :3]).any()
            respawn += int(killed[b] and s1["ALIVE"][b, 0] == 1 and s1["HP"][b, 0] == 100 and moved)
            for s0, s in ((r["posed"], s1), (s1, r["steps"][1])):
                heal += int(not killed[a] and s["HP"][a, 0] > s0["HP"][a, 0] and s0["DEBUG_AGENT_I32"][a, 8] == 0)
    assert exact >= 1 and double >= 1 and mutual >= 1 and respawn >= 1 and heal >= 1, \
        dict(exact=exact, double=double, mutual=mutual, respawn=respawn, heal=heal)


@pytest.mark.parametrize("name", ["zone", "zone_noreset"])
def test_zone_cases_cover_point_capture_change_and_match_end(name):
    point = capture = change = end = 0
    for r in records(name):
        wi0, wi1 = r["posed"]["DEBUG_WORLD_I32"], r["steps"][0]["DEBUG_WORLD_I32"]
        wf0 = r["posed"]["DEBUG_WORLD_F32"]
        point += int((wi1[:, 7] == 1).sum())
        capture += int(((wi0[:, 6] == 0) & (wi1[:, 6] == 1)).sum())
        change += int((wi1[:, 3] != wi0[:, 3]).sum())
        done = r["steps"][0]["DONE"].reshape(len(wi0), -1)
        end += int(((done == 1).all(1) & (wi0[:, 1] == P.EPISODE_LEN - 1) & (wf0[:, 0] == wf0[:, 1])).sum())
    assert point >= 1 and capture >= 1 and change >= 1 and end >= 1, dict(point=point, capture=capture,
                                                                          change=change, end=end)


def test_crumb_case_overflows_the_pool():
    r = records("crumbs")[0]
    wi0, wi1 = r["posed"]["DEBUG_WORLD_I32"], r["steps"][0]["DEBUG_WORLD_I32"]
    assert (wi0[:, 15] == P.MAX_CRUMBS - 1).all()
    assert (wi1[:, 20] > wi0[:, 20]).any(), "crumbOverflow did not rise"
    assert (wi1[:, 15] == P.MAX_CRUMBS).any()


def test_move_case_transitions_and_falls():
    r = records("move")[0]
    ai0, ai1 = r["posed"]["DEBUG_AGENT_I32"], r["steps"][0]["DEBUG_AGENT_I32"]
    af0, af1 = r["posed"]["DEBUG_AGENT_F32"], r["steps"][0]["DEBUG_AGENT_F32"]
    assert ai0[0, 2] == 1 and ai1[0, 0] == P.CROUCH and ai1[0, 1] == P.PRONE and ai1[0, 2] > 0
    assert ai1[1, 0] == P.CROUCH and ai1[1, 2] == 0
    assert (af1[4:6, 2] < af0[4:6, 2]).all(), "the lifted agents did not fall"
