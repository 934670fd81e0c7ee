"""Times k_camera (csrc/camera.hip) against k_lidar in the same run (on the GPU
box): rays per second of each, side by side.  Both walk the same octant images
of the lidar tree, so k_lidar is the yardstick for the cost of a camera ray.

Batches C2 (3v3 x 4,096) and C3 (6v6 x 16,384); camera sizes 64 x 32 and
16 x 8 at 90 degrees; LDS-resident and global-resident images; two states: the
driver window (init and 20 steps of the hash tape) and a combat state (300
more steps under the device aim-bot, mpenv_combat_actions mode 1).

k_camera: HIP events on one stream around REPS back-to-back
mpenv_camera_render calls.  k_lidar: the step's own kernel timing
(mpenv_enable_kernel_timing) over REPS steps, which moves the state on by
those steps; so within a state every variant's rounds are interleaved --
round by round, each residency and camera size in turn -- and each figure is
the median round over ROUNDS rounds after a warm-up round, with the fastest
and the slowest beside it.  A lidar ray count is 80 per agent.

usage: python tools/camera_timing.py [--batches C3,C2] [--out profiles/camera_timing.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import camera_testlib as K  # noqa: E402
import mpenv_testlib as T  # noqa: E402
import scene_residency_testlib as R  # noqa: E402

REPS, ROUNDS = 3, 5
SIZES = [(64, 32), (16, 8)]
RESIDENCIES = [("lds", R.LDS), ("global", R.GLOBAL)]
LIDAR_RAYS = 80


def stats(ms_list, rays):
    ms = statistics.median(ms_list)
    return {"ms": round(ms, 4), "ms_min": round(min(ms_list), 4), "ms_max": round(max(ms_list), 4),
            "rays": rays, "grays_per_s": round(rays / (ms * 1e-3) / 1e9, 3),
            "grays_per_s_range": [round(rays / (max(ms_list) * 1e-3) / 1e9, 3),
                                  round(rays / (min(ms_list) * 1e-3) / 1e9, 3)]}


def measure(ts, W):
    A = W * 2 * ts
    lib = K.lib()
    e = T.Engine(W, ts)
    hip = e.mem.hip
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]

    def ok(rc):
        assert rc == 0, (rc, lib.mpenv_last_error())

    st, ev0, ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(hip.hipStreamCreate(C.byref(st)))
    ok(hip.hipEventCreate(C.byref(ev0)))
    ok(hip.hipEventCreate(C.byref(ev1)))

    def lidar_ms():
        """k_lidar's mean time over REPS steps of the tape (the step's own events)."""
        names = (C.c_char_p * 16)()
        ms = (C.c_float * 16)()
        launches = (C.c_int32 * 16)()
        ok(lib.mpenv_enable_kernel_timing(e.h, 1))
        for _ in range(REPS):
            e.step()
        n = lib.mpenv_kernel_timings(e.h, 16, names, ms, launches)
        ok(lib.mpenv_enable_kernel_timing(e.h, 0))
        by = {names[k].decode(): ms[k] for k in range(n)}
        return by["k_lidar"]

    def camera_ms():
        ok(K.render(e, st))  # not timed: the first launch after a change of camera or residency
        ok(hip.hipEventRecord(ev0, st))
        for _ in range(REPS):
            ok(K.render(e, st))
        ok(hip.hipEventRecord(ev1, st))
        ok(hip.hipEventSynchronize(ev1))
        ms = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1))
        return ms.value / REPS

    e.put_ctrl([0, 1, 1])
    e.init()
    ring = e.mem.upload(T.mpenv_tape.tape_ring(1234, 0, A, 4))
    step_no = 0

    def advance(n, combat):
        nonlocal step_no
        for _ in range(n):
            slot = ring + (step_no % 4) * A * 24
            if combat:
                e.combat_actions(slot, None, 1)
            else:
                e.copy_actions(slot)
            e.step()
            step_no += 1

    out = {"workload": f"{ts}v{ts} x {W} worlds ({A} agents)", "reps_per_round": REPS, "rounds": ROUNDS,
           "camera_bytes": {f"{w}x{h}": A * w * h * 5 for w, h in SIZES}, "states": {}}
    for state, n, combat in (("driver_window", 20, False), ("combat", 300, True)):
        advance(n, combat)
        times = {(rn, key): [] for rn, _ in RESIDENCIES for key in ["k_lidar"] + [f"k_camera_{w}x{h}" for w, h in SIZES]}
        for rnd in range(ROUNDS + 1):
            for rn, mode in RESIDENCIES:
                assert R.set_residency(e, mode) == 0
                ok(K.disable(e))
                t = lidar_ms()  # camera off: the step is the parent's
                if rnd > 0:
                    times[(rn, "k_lidar")].append(t)
                for w, h in SIZES:
                    ok(K.enable(e, K.config(w, h, 90.0)))
                    t = camera_ms()
                    if rnd > 0:
                        times[(rn, f"k_camera_{w}x{h}")].append(t)
        ok(K.disable(e))
        assert R.set_residency(e, R.AUTO) == 0
        res = {}
        for rn, _ in RESIDENCIES:
            block = {"k_lidar": stats(times[(rn, "k_lidar")], A * LIDAR_RAYS)}
            for w, h in SIZES:
                key = f"k_camera_{w}x{h}"
                block[key] = stats(times[(rn, key)], A * w * h)
                block[key]["rays_per_s_over_lidar"] = round(block[key]["grays_per_s"] / block["k_lidar"]["grays_per_s"], 3)
            res[rn] = block
        out["states"][state] = res
    e.mem.free(ring)
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camera_timing.json"))
    ap.add_argument("--batches", default="C3,C2")
    args = ap.parse_args()
    shapes = {"C3": (6, 16384), "C2": (3, 4096)}
    out = {b: measure(*shapes[b]) for b in args.batches.split(",")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
