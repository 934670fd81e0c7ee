"""Reading a world checkpoint without loading it.

`SimManager.save_state` fills a device buffer of `state_bytes()` bytes with
the whole batch's state (include/mpenv.h mpenv_state_*): a
256-B header, then one section per state buffer.  This module names the
sections and views them in place:

    blob = torch.empty(sim.state_bytes(), dtype=torch.uint8, device="cuda")
    sim.save_state(blob.data_ptr())
    hp = mpenv_state.view(blob, "HP")            # [A, 1] float32, zero-copy
    px = mpenv_state.view(blob, "px")            # [A, 1] float32 (internal column)

An exported buffer's section carries the export's name (MPENV_EXPORT_*
without the prefix) and its tensor shape; every other section the engine's
name of the column and the shape (rows, elements per row).  The layout is a
pure function of (num_worlds, team_size, spawn track length) and needs no GPU.
"""
import struct
from typing import Dict, Tuple

import madrona_mp_env as _m

HEADER_BYTES = 256
MAGIC = 0x3153504D  # "MPS1"
ROW_KINDS = ("agent", "world", "team")  # rows: W * 2 * team_size, W, 2 * W

Section = Tuple[int, int, str, Tuple[int, ...]]  # offset, nbytes, dtype, shape


def _dims(sim_or_dims):
    if isinstance(sim_or_dims, (tuple, list)):
        W, team, track = sim_or_dims
        return int(W), int(team), int(track)
    return tuple(int(x) for x in sim_or_dims.state_dims())


def num_sections(sim_or_dims) -> int:
    return _m.state_section(-1, *_dims(sim_or_dims))[3]


def total_bytes(sim_or_dims) -> int:
    return _m.state_section(-1, *_dims(sim_or_dims))[2]


def sections(sim_or_dims) -> Dict[str, Section]:
    """{name: (offset, nbytes, dtype, shape)} in blob order, for a SimManager
    or a (num_worlds, team_size, spawn_track_len) tuple."""
    dims = _dims(sim_or_dims)
    out = {}
    for k in range(num_sections(dims)):
        name, off, nbytes, _rb, _kind, _eid, dtype, shape = _m.state_section(k, *dims)
        out[name] = (off, nbytes, dtype, tuple(shape))
    return out


def row_kinds(sim_or_dims) -> Dict[str, str]:
    """{name: "agent" | "world" | "team"}: what one row of the section is."""
    dims = _dims(sim_or_dims)
    return {_m.state_section(k, *dims)[0]: ROW_KINDS[_m.state_section(k, *dims)[4]]
            for k in range(num_sections(dims))}


def header(blob) -> dict:
    """The header fields of a saved blob (a torch uint8 tensor, any device)."""
    raw = bytes(blob[:48].cpu().numpy().tobytes())
    magic, version, W, N, T, track, flags, task, nbytes, nsec = struct.unpack("<IIiiiiIiqi", raw[:44])
    return dict(magic=magic, version=version, num_worlds=W, agents_per_world=N, team_size=T,
                spawn_track_len=track, sim_flags=flags, task=task, bytes=nbytes, sections=nsec)


def view(blob, name: str, dims=None):
    """Zero-copy torch view of one section of a saved blob (a contiguous
    uint8 tensor).  dims = (num_worlds, team_size, spawn_track_len); read from
    the blob's header when not given."""
    import torch

    if dims is None:
        h = header(blob)
        if h["magic"] != MAGIC:
            raise ValueError("not a state snapshot (bad magic)")
        dims = (h["num_worlds"], h["team_size"], h["spawn_track_len"])
    secs = sections(dims)
    if name not in secs:
        raise KeyError(f"no section {name!r} in a state snapshot")
    off, nbytes, dtype, shape = secs[name]
    if blob.dtype != torch.uint8 or blob.dim() != 1 or blob.numel() < off + nbytes:
        raise ValueError("blob must be a 1-D uint8 tensor of at least state_bytes() bytes")
    return blob[off:off + nbytes].view(getattr(torch, dtype)).view(shape)
