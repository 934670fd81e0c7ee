"""The step from constructed states: engine against oracle, byte for byte
(tests/posed_testlib.py; DESIGN.md §7 "Posed states").

Every other step-level test walks a rollout from spawn; these start from states
written down on purpose.  Each family brings both sides to a shared rollout
state, and per round poses the same edit on both (checked before any step: the
engine's debug gather and state exports equal the oracle's), steps twice and
compares STEP_OUTPUTS, DEBUG_OUTPUTS, the bot's action columns and the explore
cells after each step.  tests/test_posed_states.py shows on the CPU that the
families reach the branches they are meant for.

Shapes: 6v6 x 13 holds one bot per navmesh triangle (156 >= 155); 3v3 x 5 and
1v1 x 3 serve the rest."""
import ctypes as C

import pytest

import posed_testlib as P
import scene_residency_testlib as R

pytestmark = pytest.mark.gpu

FAMILIES = {
    "bots": lambda: P.BOTS,
    "combat": lambda: P.COMBAT,
    "zone": lambda: P.zone_family(rotated=False),
    "zone_rotated": lambda: P.zone_family(),
    "zone_rotated_no_auto_reset": lambda: P.zone_family(auto_reset=False),
    "move": lambda: P.MOVE,
    "crumbs": lambda: P.CRUMBS,
}


@pytest.mark.parametrize("name", list(FAMILIES))
def test_posed_family_matches_oracle(name):
    recs = P.run_family(FAMILIES[name](), engine=True)
    assert recs and all(len(r["steps"]) == 2 for r in recs)


def world_groups(e):
    n = C.c_int32(-1)
    e._ok(e.lib.mpenv_world_groups(e.h, C.byref(n)))
    return n.value


def test_posed_bots_under_three_world_groups():
    """13 worlds in three groups: group boundaries fall inside a block of agents."""
    def three(e):
        assert world_groups(e) == 3

    def setup(e):
        e.set_world_groups(3)
        three(e)

    P.run_family(P.BOTS, engine=True, setup=setup, after=three)


def test_posed_bots_from_global_resident_images():
    def is_global(e):
        assert R.residency(e) == R.GLOBAL

    def setup(e):
        assert R.set_residency(e, R.GLOBAL) == 0, e.lib.mpenv_last_error().decode()
        is_global(e)

    P.run_family(P.BOTS, engine=True, setup=setup, after=is_global)
