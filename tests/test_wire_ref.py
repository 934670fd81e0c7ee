"""tests/wire_ref.py, the NumPy statement of wire format version 1, checked
against itself: decode(encode(x)) == x on random columns, the columns do not
overlap, every offset is a multiple of 256 B, and a few offsets and bits worked
out by hand from the format's description."""
import numpy as np
import pytest

import wire_ref as R

SHAPES = [(A, W) for A in (6, 30, 150) for W in (3, 5, 15)]


def random_columns(A, W, keyframe, seed):
    rng = np.random.default_rng(seed)
    cols = {}
    for name, dt, shape in R.columns(A, W, keyframe):
        if name in ("depth", "plane0", "plane1", "packed"):
            continue
        if dt.kind == "f":  # any bit pattern but the format's own: NaN payloads and -0 must survive
            cols[name] = rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32).view(np.float32)
        elif dt.itemsize == 1:
            cols[name] = rng.integers(0, 256, shape).astype(np.uint8)
        else:
            cols[name] = rng.integers(-(1 << 31), 1 << 31, shape, dtype=np.int64).astype(np.int32)
    for n in R.PACKED:
        cols[n] = rng.integers(0, 256, A).astype(np.int32)
    cls = rng.integers(0, 4, (A, R.RAYS))
    lidar = np.zeros((A, R.RAYS, 4), np.float32)
    lidar[..., 0] = np.where(cls == 0, -1.0, rng.uniform(0, 1000, (A, R.RAYS))).astype(np.float32)
    for c in (1, 2, 3):
        lidar[..., c] = cls == c
    cols["lidar"] = lidar
    return cols


@pytest.mark.parametrize("keyframe", [False, True])
@pytest.mark.parametrize("A,W", SHAPES)
def test_decode_inverts_encode(A, W, keyframe):
    cols = random_columns(A, W, keyframe, 1000 * A + 10 * W + keyframe)
    header = R.make_header(A, W, 6, 3, keyframe, world_offset=64)
    msg, mask = R.encode(cols, header)
    assert len(msg) == R.layout(A, W, keyframe)["total"] == header["bytes"]
    got_header, got = R.decode(msg)
    assert got_header == header
    for name, a in cols.items():
        b = got[name]
        assert a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize, name
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), name
    assert (msg[mask == 0] == 0).all()
    assert keyframe == ("lkObs" in got)


@pytest.mark.parametrize("keyframe", [False, True])
@pytest.mark.parametrize("A,W", SHAPES)
def test_columns_are_aligned_and_do_not_overlap(A, W, keyframe):
    L = R.layout(A, W, keyframe)
    end = R.HEADER_BLOCK
    covered = np.zeros(L["total"], np.int32)
    covered[:R.HEADER_BLOCK] += 1
    for name, v in L.items():
        if name == "total":
            continue
        off, nbytes, dt, shape = v
        assert off % 256 == 0 and off >= end, name  # wire order, no overlap
        assert nbytes == int(np.prod(shape)) * dt.itemsize > 0, name
        covered[off:off + nbytes] += 1
        end = off + nbytes
    assert covered.max() == 1
    assert L["total"] % 256 == 0 and 0 <= L["total"] - end < 256
    assert [n for n in L if n != "total"] == [c[0] for c in R.columns(A, W, keyframe)]


def test_hand_computed_layout_and_bits():
    # 1v1 x 3: A = 6, W = 3.  Every [A] or [W] column is one 256-B block: 15 AF +
    # hp, alive, reward + 3 AI + done = 22 blocks after the header
    L = R.layout(6, 3, False)
    assert L["px"][0] == 256 and L["hp"][0] == 256 * 16 and L["done"][0] == 256 * 22
    assert L["magazine"][:2] == (256 * 23, 48) and L["packed"][0] == 256 * 24
    assert L["visMask"][:2] == (256 * 25, 6) and L["rewardCoefs"][:2] == (256 * 26, 216)
    assert L["depth"][:2] == (256 * 27, 1920)          # 480 rays, 7.5 blocks -> 8
    assert L["plane0"][:2] == (256 * 35, 60) and L["plane1"][0] == 256 * 36  # 15 words
    assert L["curStep"][0] == 256 * 37 and L["episodeCounter"][0] == 256 * 46
    assert L["matchResult"][:2] == (256 * 47, 360)     # 2 blocks
    assert L["total"] == 256 * 49
    K = R.layout(6, 3, True)
    assert K["lkObs"][:2] == (256 * 49, 6 * 6 * 32 * 4) and K["lkPos"][0] == 256 * 49 + 4608
    assert K["total"] == 256 * 49 + 4608 + 512         # lkPos: 432 B -> 2 blocks
    # ~477 B per agent + 160 B per world, DESIGN.md §6 (the unpadded payload)
    big = R.columns(196608, 16384, False)
    payload = sum(int(np.prod(s)) * d.itemsize for _, d, s in big)
    assert payload == 196608 * 477 + 16384 * 160
    # the class bits of ray 37 of agent 1 (r = 117): bit 21 of word 3
    lidar = np.zeros((2, 80, 4), np.float32)
    lidar[..., 0] = -1
    lidar[1, 37] = (12.5, 0, 0, 1)   # opponent: both planes
    lidar[0, 0] = (3.0, 1, 0, 0)     # wall: plane 0 only
    lidar[1, 79] = (4.0, 0, 1, 0)    # teammate: plane 1 only, the last ray (r = 159: bit 31 of word 4)
    depth, p0, p1 = R.lidar_split(lidar)
    assert p0.tolist() == [1, 0, 0, 1 << 21, 0] and p1.tolist() == [0, 0, 0, 1 << 21, 1 << 31]
    assert depth[117] == 12.5 and depth[1] == -1
    assert R.pack_word(2, 1, 3, 36).item() == 2 | 1 << 8 | 3 << 16 | 36 << 24
    with pytest.raises(ValueError):
        lidar[0, 5] = (0.5, 1, 1, 0)
        R.lidar_split(lidar)
    # header bytes
    msg, mask = R.encode(random_columns(6, 3, False, 0), R.make_header(6, 3, 2, 1, False, world_offset=64))
    assert msg[:4].tobytes() == b"MPW1" and mask[:48].all() and not mask[48:256].any()
    assert msg[4:16].view(np.uint32).tolist() == [1, 0, 64]
    assert msg[16:32].view(np.int32).tolist() == [3, 2, 1, 0]
    assert msg[32:48].view(np.int64).tolist() == [6, 256 * 49]
