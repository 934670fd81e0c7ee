"""bench.py --dump-outputs (CPU): what dump_outputs writes for a set of
world-major tensors -- dtypes, the byte budget, and that the sampled worlds
are the same for every tensor and from call to call."""
import os
import sys

import numpy as np
import torch

import mpenv_testlib as T

sys.path.insert(0, T.ROOT)
import bench  # noqa: E402


def _tensors(W, N):
    g = torch.Generator().manual_seed(3)
    world = torch.arange(W, dtype=torch.int32)
    return {
        "obs": torch.randn(W * N, 7, 5, generator=g),  # per agent, float
        "agent_world": world.repeat_interleave(N).reshape(W * N, 1),  # per agent, int
        "world": world.reshape(W, 1),  # per world, int
        "bits": (world + 0x7FFFFFF0).view(torch.uint32).reshape(W, 1),  # wraps past 2^31 as int32
        "odd": torch.randn(5, generator=g),  # not world-major: written whole
    }


def test_dump_samples_whole_worlds_within_the_budget(tmp_path, monkeypatch):
    W, N = 300, 4
    t = _tensors(W, N)
    monkeypatch.setattr(bench, "DUMP_BUDGET", 16 << 10)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, t, W)
    bench.dump_outputs(b, t, W)
    assert sorted(os.listdir(a)) == sorted(n + ".npy" for n in t)
    out = {n: np.load(os.path.join(a, n + ".npy")) for n in t}
    for n in t:  # the same rows from call to call
        assert out[n].tobytes() == np.load(os.path.join(b, n + ".npy")).tobytes(), n
    assert sum(x.nbytes for x in out.values()) <= 16 << 10
    assert out["obs"].dtype == np.float32 and out["odd"].dtype == np.float32
    assert out["world"].dtype == np.float64 and out["agent_world"].dtype == np.float64
    worlds = out["world"][:, 0].astype(np.int64)
    assert 1 < len(worlds) < W and (np.diff(worlds) > 0).all()
    # every tensor keeps the same worlds, each with all of its rows
    assert (out["agent_world"][:, 0] == np.repeat(worlds, N)).all()
    rows = (worlds[:, None] * N + np.arange(N)).ravel()
    assert out["obs"].tobytes() == t["obs"][rows].numpy().tobytes()
    assert (out["bits"][:, 0] == worlds + 0x7FFFFFF0).all()  # unsigned, not wrapped
    assert out["odd"].tobytes() == t["odd"].numpy().tobytes()


def test_dump_writes_everything_when_it_fits(tmp_path):
    W, N = 6, 2
    t = _tensors(W, N)
    bench.dump_outputs(str(tmp_path), t, W)
    for n, x in t.items():
        got = np.load(os.path.join(str(tmp_path), n + ".npy"))
        assert got.shape == tuple(x.shape), n
    assert (np.load(os.path.join(str(tmp_path), "world.npy"))[:, 0] == np.arange(W)).all()
