"""The world-checkpoint blob's layout (include/mpenv.h mpenv_state_section,
csrc/state.hip) without a GPU: alignment, order, sizes from the row kinds,
which exports are inside, 64-bit offsets at 131,072 worlds, and the Python
views of mpenv_state over a fake CPU blob."""
import ctypes as C

import numpy as np
import pytest

import mpenv_testlib as T

CONFIGS = [(3, 1), (5, 3), (3, 6), (16384, 6), (131072, 6)]
TRACK = 128
# exports that are views of a buffer-table buffer (csrc/engine.h MP_BUFS): the
# reference's ids less the alias of AGENT_MAP and the two event-log buffers
TABLE_EXPORTS = {n: i for n, i in T.EXPORT.items()
                 if i < 40 and n not in ("UNMASKED_AGENT_MAP", "EVENT_LOG", "PACKED_STEP_SNAPSHOT")}
# documented exemptions (csrc/state.hip kStateExempt): constant zeros; and
# SIM_CONTROL, the unsliced trainCtrl row
EXEMPT = {"AGENT_MAP"}
ELEM = {0: 4, 1: 4, 2: 4, 3: 1, 4: 2, 5: 8}


def all_sections(W, team, track=TRACK):
    blob = T.state_section(-1, W, team, track)
    secs = [T.state_section(k, W, team, track) for k in range(blob["row_bytes"])]
    assert all(s is not None for s in secs)
    assert T.state_section(blob["row_bytes"], W, team, track) is None  # one past the end
    return blob, secs


def rows(kind, W, team):
    return {0: W * 2 * team, 1: W, 2: 2 * W}[kind]


@pytest.mark.parametrize("W,team", CONFIGS)
def test_sections_are_aligned_ordered_and_sized_by_their_rows(W, team):
    blob, secs = all_sections(W, team)
    assert blob["offset"] == 0 and blob["kind"] == -1
    end = 256  # the header
    for s in secs:
        assert s["offset"] % 256 == 0, s
        assert s["offset"] >= end, s  # ordered, no overlap
        assert s["offset"] - end < 256, s  # and no gap beyond the alignment
        assert s["bytes"] == rows(s["kind"], W, team) * s["row_bytes"], s
        assert s["bytes"] > 0
        end = s["offset"] + s["bytes"]
    assert end == blob["bytes"]
    assert len({s["name"] for s in secs}) == len(secs)


@pytest.mark.parametrize("W,team", CONFIGS)
def test_every_table_export_is_inside_exactly_once(W, team):
    lib = T.lib_mpenv()
    _, secs = all_sections(W, team)
    by_id = {}
    for s in secs:
        if s["export_id"] >= 0:
            by_id.setdefault(s["export_id"], []).append(s)
    for name, eid in TABLE_EXPORTS.items():
        if name in EXEMPT:
            assert eid not in by_id, name
            continue
        assert len(by_id.get(eid, [])) == 1, name
        s = by_id[eid][0]
        assert s["name"] == name
        dt, nd = C.c_int32(), C.c_int32()
        dims = (C.c_int64 * 8)()
        assert lib.mpenv_export_layout(eid, W, team, C.byref(dt), C.byref(nd), dims) == 0
        assert dims[0] == rows(s["kind"], W, team), name
        assert s["row_bytes"] == 4 * int(np.prod([dims[i] for i in range(1, nd.value)])), name
    assert T.EXPORT["SIM_CONTROL"] not in by_id and T.EXPORT["UNMASKED_AGENT_MAP"] not in by_id
    assert set(by_id) == {i for n, i in TABLE_EXPORTS.items() if n not in EXEMPT}


def test_offsets_beyond_4_gib_are_exact():
    """6v6 x 131,072: the layout recomputed with Python integers."""
    W, team = 131072, 6
    blob, secs = all_sections(W, team)
    off = 256
    for s in secs:
        assert s["offset"] == off, s
        nbytes = rows(s["kind"], W, team) * s["row_bytes"]
        assert s["bytes"] == nbytes
        off = (off + nbytes + 255) // 256 * 256
    assert blob["bytes"] == secs[-1]["offset"] + secs[-1]["bytes"] > 2 ** 32
    assert sum(s["offset"] > 2 ** 32 for s in secs) > 10


def test_state_columns_and_hand_allocated_buffers_are_sections():
    W, team = 5, 3
    _, secs = all_sections(W, team)
    by = {s["name"]: s for s in secs}
    for col in ("px", "rngCtr", "wRngA", "episodeCounter", "teamRew0"):
        assert by[col]["row_bytes"] == 4
    for k in range(6):
        assert by[f"dmg{k}"]["bytes"] == W * 2 * team * 4
    assert by["resetKeys"]["row_bytes"] == 11 * 8
    assert by["visMask"]["row_bytes"] == 1 and by["visOcc"]["row_bytes"] == 2 * team * 4
    assert by["spawnTrack"]["row_bytes"] == 3 * TRACK * 4
    longer = {s["name"]: s for s in all_sections(W, team, 200)[1]}
    assert longer["spawnTrack"]["row_bytes"] == 3 * 200 * 4


def test_bad_arguments_are_refused():
    lib = T.lib_mpenv()
    for args in ((0, 0, 3, TRACK), (0, 3, 0, TRACK), (0, 3, 7, TRACK), (0, 3, 3, 127), (-2, 3, 3, TRACK)):
        assert T.state_section(*args) is None, args
        assert lib.mpenv_last_error()


@pytest.mark.parametrize("W,team", CONFIGS[:3])
def test_python_views_of_a_cpu_blob(W, team):
    import torch

    import mpenv_state

    blob_info, secs = all_sections(W, team)
    dims = (W, team, TRACK)
    assert mpenv_state.total_bytes(dims) == blob_info["bytes"]
    table = mpenv_state.sections(dims)
    assert list(table) == [s["name"] for s in secs]
    # a fake blob: byte i holds i mod 251, so a view's bytes tell its offset
    blob = (torch.arange(blob_info["bytes"], dtype=torch.int64) % 251).to(torch.uint8)
    raw = blob.numpy()
    lib = T.lib_mpenv()
    for k, s in enumerate(secs):
        off, nbytes, dtype, shape = table[s["name"]]
        assert (off, nbytes) == (s["offset"], s["bytes"])
        dt = C.c_int32()
        assert lib.mpenv_state_section_dtype(k, C.byref(dt)) == 0
        assert int(np.prod(shape)) * ELEM[dt.value] == nbytes, s
        assert shape[0] == rows(s["kind"], W, team)
        v = mpenv_state.view(blob, s["name"], dims)
        assert tuple(v.shape) == shape and str(v.dtype) == "torch." + dtype
        assert v.untyped_storage().data_ptr() == blob.untyped_storage().data_ptr()  # zero-copy
        assert np.array_equal(v.contiguous().view(torch.uint8).numpy().reshape(-1), raw[off:off + nbytes])
    assert table["SELF_POSITION"][3] == (W * 2 * team, 3) and table["SELF_POSITION"][2] == "float32"
    assert table["MATCH_RESULT"][3] == (W, 30) and table["MATCH_RESULT"][2] == "int32"
    with pytest.raises(KeyError):
        mpenv_state.view(blob, "AGENT_MAP", dims)
