"""Wire format version 1 ("MPW1") of the learner exchange, stated in NumPy.

Written from the format's description (the header comment of
csrc/wire.hip and its WireHeader), not from the kernels: nothing here calls
into the library, so a test that compares the pack kernel's bytes with
encode() (or the unpack kernel's outputs with decode()) checks each kernel by
itself against an independent statement of the format.

A message:
  * a 256-B header block whose first 80 B are the header
      u32 magic "MPW1", u32 version 1, u32 flags (1 keyframe, 2 overflow),
      u32 worldOffset, i32 W, i32 N, i32 T, i32 pad (0), i64 A, i64 bytes,
      u32 reserved[8]
    -- the sender defines the first 48 B; the reserved words and the rest of
    the block are not part of the format;
  * then structure-of-arrays columns, each starting at a multiple of 256 B
    (a column's length is rounded up to 256 B; the padding is undefined), in
    this order: the 15 f32 agent columns AF, hp, alive, reward, the 3 i32
    agent columns AI, done, magazine [A][2], the packed word [A]
    (curPose | tgtPose << 8 | weapon << 16 | flags << 24), the visibility
    byte [A], the reward coefficients [A][9], the lidar depth [A * 80], the
    two class bit-planes, the 10 i32 world columns WI, the episode results
    [W][30] and, in a keyframe only, the last-known rows [A][6][32] and
    [A][6][3];
  * the lidar: ray r = agent * 80 + k, the 64 forward rays first, then the
    16 rear rays; depth[r] is the ray's first float, its class c (0 none,
    1 wall, 2 teammate, 3 opponent) is bit (r & 31) of word (r >> 5) of
    plane 0 (c & 1) and plane 1 (c >> 1); the f32 row is
    (depth, c == 1, c == 2, c == 3).
"""
import struct

import numpy as np

MAGIC = 0x3157504D  # "MPW1", little-endian
VERSION = 1
FLAG_KEYFRAME, FLAG_OVERFLOW = 1, 2
HEADER_BLOCK = 256
HEADER_FMT = "<IIIIiiiiqq"  # the 48 defined bytes
HEADER_FIELDS = ("magic", "version", "flags", "worldOffset", "W", "N", "T", "pad", "A", "bytes")
ALIGN = 256
FWD_RAYS, REAR_RAYS = 64, 16
RAYS = FWD_RAYS + REAR_RAYS

AF = ("px", "py", "pz", "vx", "vy", "vz", "rw", "rx", "ry", "rz", "ayaw", "apitch", "dyv", "dpv", "firedT")
AI = ("transRem", "wasShot", "autohealSteps")
WI = ("curStep", "filtMatched0", "filtMatched1", "curZone", "controlling", "contested", "captured",
      "stepsUntilPoint", "zoneSteps", "episodeCounter")
PACKED = ("curPose", "tgtPose", "weapon", "flags")  # byte 0..3 of the packed word


def columns(A, W, keyframe):
    """[(name, dtype, shape)] in wire order."""
    f4, i4, u4 = np.dtype("<f4"), np.dtype("<i4"), np.dtype("<u4")
    words = (A * RAYS + 31) // 32
    cols = [(n, f4, (A,)) for n in AF]
    cols += [("hp", f4, (A,)), ("alive", f4, (A,)), ("reward", f4, (A,))]
    cols += [(n, i4, (A,)) for n in AI]
    cols += [("done", i4, (A,)), ("magazine", i4, (A, 2)), ("packed", u4, (A,)), ("visMask", np.dtype("u1"), (A,)),
             ("rewardCoefs", f4, (A, 9)), ("depth", f4, (A * RAYS,)), ("plane0", u4, (words,)),
             ("plane1", u4, (words,))]
    cols += [(n, i4, (W,)) for n in WI]
    cols += [("matchResult", i4, (W, 30))]
    if keyframe:
        cols += [("lkObs", f4, (A, 6, 32)), ("lkPos", f4, (A, 6, 3))]
    return cols


def layout(A, W, keyframe):
    """{column: (offset, nbytes, dtype, shape)} in wire order, and the
    message's total length under "total"."""
    out = {}
    off = HEADER_BLOCK
    for name, dt, shape in columns(A, W, keyframe):
        nbytes = int(np.prod(shape)) * dt.itemsize
        out[name] = (off, nbytes, dt, shape)
        off += -(-nbytes // ALIGN) * ALIGN
    out["total"] = off
    return out


def column_items(L):
    """layout()'s entries without the total."""
    return [(n, v) for n, v in L.items() if n != "total"]


def pack_word(cur_pose, tgt_pose, weapon, flags):
    v = [np.asarray(x).astype(np.int64).astype(np.uint32) for x in (cur_pose, tgt_pose, weapon, flags)]
    return v[0] | (v[1] << np.uint32(8)) | (v[2] << np.uint32(16)) | (v[3] << np.uint32(24))


def lidar_split(lidar):
    """[A][80][4] f32 rows -> (depth [A * 80] f32, plane0, plane1 u32 words)."""
    lidar = np.ascontiguousarray(lidar, np.float32)
    A = lidar.shape[0]
    assert lidar.shape == (A, RAYS, 4)
    flat = lidar.reshape(A * RAYS, 4)
    bits = flat[:, 1:].view(np.uint32)
    one = np.uint32(0x3F800000)
    hot = bits == one
    zero = bits == 0
    cls = np.zeros(A * RAYS, np.uint32)
    for c in (1, 2, 3):  # exactly channel c is 1.0f and the other two are +0
        cls[hot[:, c - 1] & np.delete(zero, c - 1, axis=1).all(axis=1)] = c
    none = zero.all(axis=1) & (flat[:, 0].view(np.uint32) == np.uint32(0xBF800000))  # (-1, 0, 0, 0)
    if not ((cls > 0) | none).all():
        raise ValueError("a lidar ray is neither (t, one-hot) nor (-1, 0, 0, 0): the format cannot carry it")
    words = (A * RAYS + 31) // 32
    planes = []
    for p in range(2):
        bit = np.zeros(words * 32, np.uint32)
        bit[:A * RAYS] = (cls >> np.uint32(p)) & np.uint32(1)
        planes.append((bit.reshape(words, 32) << np.arange(32, dtype=np.uint32)).sum(axis=1, dtype=np.uint32))
    return flat[:, 0].copy(), planes[0], planes[1]


def lidar_join(depth, plane0, plane1, A):
    """The inverse: [A][80][4] f32 rows."""
    r = np.arange(A * RAYS)
    cls = ((plane0[r >> 5] >> (r & 31).astype(np.uint32)) & np.uint32(1)) | \
          (((plane1[r >> 5] >> (r & 31).astype(np.uint32)) & np.uint32(1)) << np.uint32(1))
    out = np.zeros((A * RAYS, 4), np.float32)
    out[:, 0] = depth
    for c in (1, 2, 3):
        out[:, c] = (cls == c).astype(np.float32)
    return out.reshape(A, RAYS, 4)


def make_header(A, W, N, T, keyframe, world_offset=0, overflow=False):
    return dict(magic=MAGIC, version=VERSION,
                flags=(FLAG_KEYFRAME if keyframe else 0) | (FLAG_OVERFLOW if overflow else 0),
                worldOffset=world_offset, W=W, N=N, T=T, pad=0, A=A, bytes=layout(A, W, keyframe)["total"])


def encode(cols, header):
    """(message bytes u8 [total], mask u8 [total]: 1 where the format defines
    the byte).  cols: {name: array} for every column of columns() except
    depth / plane0 / plane1 and packed, which come from cols["lidar"]
    ([A][80][4], forward rays first) and cols[curPose / tgtPose / weapon /
    flags]; undefined bytes of the message are left 0."""
    A, W = int(header["A"]), int(header["W"])
    keyframe = bool(header["flags"] & FLAG_KEYFRAME)
    L = layout(A, W, keyframe)
    assert header["bytes"] == L["total"]
    msg = np.zeros(L["total"], np.uint8)
    mask = np.zeros(L["total"], np.uint8)
    raw = struct.pack(HEADER_FMT, *(int(header[f]) for f in HEADER_FIELDS))
    msg[:len(raw)] = np.frombuffer(raw, np.uint8)
    mask[:len(raw)] = 1
    vals = dict(cols)
    vals["depth"], vals["plane0"], vals["plane1"] = lidar_split(cols["lidar"])
    vals["packed"] = pack_word(*(np.asarray(cols[n]).reshape(A) for n in PACKED))
    for name, (off, nbytes, dt, shape) in column_items(L):
        a = np.ascontiguousarray(np.asarray(vals[name]).reshape(shape))
        same_kind = a.dtype.kind == dt.kind or (a.dtype.kind in "iu" and dt.kind in "iu")
        assert a.dtype.itemsize == dt.itemsize and same_kind, (name, a.dtype)
        msg[off:off + nbytes] = a.view(np.uint8).reshape(-1)
        mask[off:off + nbytes] = 1
    return msg, mask


def decode(msg):
    """(header dict, {name: array}) of a message: every column of columns(),
    plus "lidar" [A][80][4] rebuilt from the depth and the planes and the
    four small integers split out of the packed word."""
    msg = np.ascontiguousarray(msg, np.uint8)
    header = dict(zip(HEADER_FIELDS, struct.unpack(HEADER_FMT, msg[:struct.calcsize(HEADER_FMT)].tobytes())))
    assert header["magic"] == MAGIC and header["version"] == VERSION, header
    A, W = header["A"], header["W"]
    L = layout(A, W, bool(header["flags"] & FLAG_KEYFRAME))
    assert header["bytes"] == L["total"] <= len(msg), (header, L["total"], len(msg))
    out = {}
    for name, (off, nbytes, dt, shape) in column_items(L):
        out[name] = msg[off:off + nbytes].view(dt).reshape(shape).copy()
    out["lidar"] = lidar_join(out["depth"], out["plane0"], out["plane1"], A)
    for k, n in enumerate(PACKED):
        out[n] = ((out["packed"] >> np.uint32(8 * k)) & np.uint32(0xFF)).astype(np.int32)
    return header, out
