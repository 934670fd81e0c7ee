"""The engine's export layout (dtype and dims of every export id) against the
oracle's, without a GPU: mpenv_export_layout is the pure half of
mpenv_export_tensor (csrc/manager.cpp exportLayout, fed by the buffer table
of csrc/engine.h)."""
import ctypes as C

import pytest

import mpenv_testlib as T

W = 3
# oracle_set_log_modes(record, replay, events) under which the oracle owns the buffer
LOG_MODES = {"RECORD_LOG": (1, 0, 1), "EVENT_LOG": (1, 0, 1), "PACKED_STEP_SNAPSHOT": (1, 0, 1),
             "SNAPSHOT_WRITTEN": (1, 0, 1), "REPLAY_LOG": (0, 1, 0)}


def engine_layout(export_id, num_worlds, team_size):
    lib = T.lib_mpenv()
    dt, nd = C.c_int32(-1), C.c_int32(-1)
    dims = (C.c_int64 * 8)()
    rc = lib.mpenv_export_layout(export_id, num_worlds, team_size, C.byref(dt), C.byref(nd), dims)
    return rc, dt.value, tuple(dims[i] for i in range(max(nd.value, 0)))


@pytest.fixture(scope="module", params=range(1, 7))
def oracles(request):
    """team size, and one Oracle(3, ts) per log-mode setting the ids need"""
    ts = request.param
    made = {}
    for modes in [None] + sorted(set(LOG_MODES.values())):
        o = T.Oracle(W, ts)
        if modes:
            o.lib.oracle_set_log_modes(o.h, *modes)
        made[modes] = o
    yield ts, made
    for o in made.values():
        o.close()


def test_export_layout_equals_the_oracles(oracles):
    ts, made = oracles
    for name, export_id in T.EXPORT.items():
        v = made[LOG_MODES.get(name)].view(name)
        rc, dt, dims = engine_layout(export_id, W, ts)
        assert rc == 0, (name, T.lib_mpenv().mpenv_last_error())
        assert T.DTYPES[dt] == v.dtype.type, name
        assert dims == v.shape, name


def test_export_layout_rejects_unknown_ids_and_bad_sizes():
    known = set(T.EXPORT.values())
    unknown = next(i for i in range(1, 200) if i not in known)
    for args in ((unknown, W, 3), (-1, W, 3), (T.EXPORT["HP"], 0, 3), (T.EXPORT["HP"], W, 0),
                 (T.EXPORT["HP"], W, 7)):
        rc, _, _ = engine_layout(*args)
        assert rc != 0, args
