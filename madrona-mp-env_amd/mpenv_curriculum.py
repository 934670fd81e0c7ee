"""Curriculum snapshots on the host (include/mpenv_curriculum.h, DESIGN.md §2
definition 21).  numpy only.

A snapshot is the reference's CurriculumSnapshot, 176 bytes: the match state
(step, zone, controller or -1, zone steps remaining, steps until the next
point) and twelve packed players.  A curriculum_data_path file is a bare array
of them, and so is every row of the live pool (SimManager.curriculum_pool(),
uint8 [R, capacity, 176]): to_file writes either, from_file reads it back, and
a file written here can be given as curriculum_data_path or to
SimManager.curriculum_pool_set."""
import numpy as np

PLAYER = np.dtype([("pos", "<i2", 3), ("yaw", "<i2"), ("pitch", "<i2"), ("mag", "u1"), ("reloading", "u1"),
                   ("hp", "u1"), ("flags", "u1")])
SNAPSHOT = np.dtype([("step", "<u2"), ("cur_zone", "u1"), ("controller", "i1"), ("zone_steps_remaining", "<u2"),
                     ("steps_until_point", "<u2"), ("players", PLAYER, 12)])
assert PLAYER.itemsize == 14 and SNAPSHOT.itemsize == 176

FLAG_FIRED, FLAG_CROUCH, FLAG_PRONE = 2, 4, 8
NEED_CAPTURED, NEED_CONTESTED, NEED_BOTH_ALIVE = 1, 2, 4


def as_snapshots(pool):
    """A flat SNAPSHOT view of `pool`: SNAPSHOT records of any shape, or uint8 [..., 176] (a pool, a
    row of it, or one snapshot's bytes)."""
    a = np.asarray(pool)
    if a.dtype == SNAPSHOT:
        return a.reshape(-1)
    if a.dtype != np.uint8 or a.ndim < 1 or a.shape[-1] != SNAPSHOT.itemsize:
        raise ValueError("pool must be SNAPSHOT records or uint8 [..., 176]")
    return np.ascontiguousarray(a).view(SNAPSHOT).reshape(-1)


def to_file(pool, path):
    """Writes the snapshots as a bare array (the curriculum_data_path format); returns their number."""
    s = as_snapshots(pool)
    s.tofile(path)
    return len(s)


def from_file(path):
    """The snapshots of a curriculum_data_path file; trailing bytes short of a snapshot are ignored, as
    the loader ignores them."""
    raw = np.fromfile(path, np.uint8)
    n = len(raw) // SNAPSHOT.itemsize
    return raw[:n * SNAPSHOT.itemsize].view(SNAPSHOT).copy()


def describe(pool, team_size=6, step_bins=10, episode_len=3000):
    """What a pool holds: dict(count, step (histogram over step_bins equal bins of [0, episode_len)),
    step_edges, zone (count per zone id, as far as the largest one present), controller (counts of
    -1, 0, 1), living (count per number of players with hp > 0, 0..2 * team_size), living_team
    ([2, team_size + 1]: the same per team))."""
    s = as_snapshots(pool)
    n = 2 * team_size
    step, edges = np.histogram(s["step"], bins=step_bins, range=(0, episode_len))
    alive = s["players"]["hp"][:, :n] > 0
    per_team = np.stack([alive[:, :team_size].sum(1), alive[:, team_size:].sum(1)])
    return dict(
        count=len(s),
        step=step,
        step_edges=edges,
        zone=np.bincount(s["cur_zone"], minlength=1),
        controller=np.array([(s["controller"] == c).sum() for c in (-1, 0, 1)]),
        living=np.bincount(alive.sum(1), minlength=n + 1),
        living_team=np.stack([np.bincount(t, minlength=team_size + 1) for t in per_team]),
    )
