"""Times the world-checkpoint kernels (csrc/state.hip) on the C3 batch, 6v6 x
16,384 (run on the GPU box): save, full load, mapped loads that restore 1 %,
10 % and 100 % of the worlds from their own snapshot worlds, a 10 % load from
random snapshot worlds, and in the same process one hipMemcpyAsync
device-to-device copy of a contiguous buffer of the snapshot's size.

HIP events on one stream around REPS back-to-back calls, the variants
interleaved over ROUNDS rounds (after a warm-up round); each figure is the
median round.  bytes_copied is the payload a call copies (it is read once and
written once, so the memory traffic is twice that); tb_per_s is payload over
time, for the checkpoint calls and the plain copy alike.

usage: python tools/state_timing.py [--out profiles/state_timing.json] [--worlds 16384] [--team 6]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mpenv_testlib as T  # noqa: E402

REPS, ROUNDS = 5, 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_timing.json"))
    ap.add_argument("--worlds", type=int, default=16384)
    ap.add_argument("--team", type=int, default=6)
    args = ap.parse_args()
    ts, W = args.team, args.worlds
    N = 2 * ts
    A = W * N
    lib = T.lib_mpenv()
    e = T.Engine(W, ts)
    hip = e.mem.hip
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]

    def ok(rc):
        assert rc == 0, (rc, lib.mpenv_last_error())

    st, ev0, ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(hip.hipStreamCreate(C.byref(st)))
    ok(hip.hipEventCreate(C.byref(ev0)))
    ok(hip.hipEventCreate(C.byref(ev1)))

    # a state worth copying: 40 steps of the action tape after init
    e.put_ctrl([0, 1, 1])
    e.init()
    ring = e.mem.upload(T.mpenv_tape.tape_ring(1234, 0, A, 8))
    for s in range(40):
        e.copy_actions(ring + (s % 8) * A * 24)
        e.step()
    nbytes = e.state_bytes()

    def dev_alloc(size):
        p = C.c_void_p()
        ok(hip.hipMalloc(C.byref(p), size))
        return p.value

    blob, plain_src, plain_dst = dev_alloc(nbytes), dev_alloc(nbytes), dev_alloc(nbytes)
    ok(lib.mpenv_state_save(e.h, blob, st))
    ok(hip.hipStreamSynchronize(st))

    rng = np.random.default_rng(11)

    def world_map(fraction, random_sources):
        m = np.full(W, -1, np.int32)
        k = max(1, int(round(W * fraction)))
        d = np.sort(rng.choice(W, k, replace=False))
        m[d] = rng.integers(0, W, k) if random_sources else d
        return e.mem.upload(m), k

    maps = {"load_map_1pct": world_map(0.01, False), "load_map_10pct": world_map(0.10, False),
            "load_map_100pct": world_map(1.0, False), "load_map_10pct_random": world_map(0.10, True)}
    calls = {"save": (lambda: lib.mpenv_state_save(e.h, blob, st), W),
             "load_full": (lambda: lib.mpenv_state_load(e.h, blob, None, st), W),
             "memcpy_d2d": (lambda: hip.hipMemcpyAsync(plain_dst, plain_src, nbytes, 3, st), W)}
    for name, (dmap, k) in maps.items():
        calls[name] = ((lambda dm=dmap: lib.mpenv_state_load(e.h, blob, dm, st)), k)

    times = {name: [] for name in calls}
    for rnd in range(ROUNDS + 1):
        for name, (fn, _) in calls.items():
            ok(hip.hipEventRecord(ev0, st))
            for _ in range(REPS):
                ok(fn())
            ok(hip.hipEventRecord(ev1, st))
            ok(hip.hipEventSynchronize(ev1))
            ms = C.c_float()
            ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1))
            if rnd > 0:  # round 0 warms every variant up
                times[name].append(ms.value / REPS)
    err = e.state_error()
    assert err == 0, err  # a refused load is a no-op and times nothing

    out = {"workload": f"{ts}v{ts} x {W} worlds after 40 tape steps", "state_bytes": nbytes,
           "sections": 0, "reps_per_round": REPS, "rounds": ROUNDS, "calls": {}}
    out["sections"] = T.state_section(-1, W, ts, 128)["row_bytes"]
    for name, (_, k) in calls.items():
        ms = statistics.median(times[name])
        copied = nbytes if k == W else int(nbytes * k / W)
        out["calls"][name] = {"ms": round(ms, 4), "ms_min": round(min(times[name]), 4),
                              "ms_max": round(max(times[name]), 4), "worlds": k, "bytes_copied": copied,
                              "tb_per_s": round(copied / (ms * 1e-3) / 1e12, 3)}
    base = out["calls"]["memcpy_d2d"]["ms"]
    full = out["calls"]["load_full"]["ms"]
    out["save_rate_vs_memcpy"] = round(base / out["calls"]["save"]["ms"], 3)
    out["load_full_rate_vs_memcpy"] = round(base / full, 3)
    out["load_1pct_vs_full"] = round(out["calls"]["load_map_1pct"]["ms"] / full, 4)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
