"""Per-kernel step time of the two scene residencies (DESIGN.md §3 "Scene
residency", §4) on the C3 batch, 6v6 x 16,384 (run on the GPU box):

  simple_map, LDS-resident             (the shipped path)
  simple_map, forced global-resident   (the price of the path on equal work)
  pillar_scene(n=100), global-resident
  pillar_scene(n=400), global-resident

Each configuration is its own manager: WARMUP steps, then STEPS timed steps
with mpenv_enable_kernel_timing (HIP events around every kernel; the step
graph is off while timing), actions from the device aim-bot over the hash tape
(mpenv_combat_actions mode 1) so that fights, shots and respawns happen.  The
figures are mpenv_kernel_timings' averages over the timed steps.

usage: python tools/scene_residency_timing.py [--out profiles/scene_residency_timing.json]
                                              [--worlds 16384] [--team 6] [--steps 200] [--warmup 100]"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import big_scene  # noqa: E402
import mpenv_testlib as T  # noqa: E402
import scene_residency_testlib as R  # noqa: E402


def run(scene, mode, ts, W, warmup, steps):
    A = W * 2 * ts
    e = T.Engine(W, ts, sim_flags=1, scene=scene)
    lib = e.lib
    if mode is not None:
        assert R.set_residency(e, mode) == 0, lib.mpenv_last_error()
    e.put_ctrl([0, 1, 1])
    e.init()
    ring = e.mem.upload(T.mpenv_tape.tape_ring(1234, 0, A, 8))

    def step(s):
        e.combat_actions(ring + (s % 8) * A * 24, None, mode=1)
        e.step()

    for s in range(warmup):
        step(s)
    assert lib.mpenv_enable_kernel_timing(e.h, 1) == 0
    for s in range(warmup, warmup + steps):
        step(s)
    names = (C.c_char_p * 16)()
    ms = (C.c_float * 16)()
    launches = (C.c_int32 * 16)()
    n = lib.mpenv_kernel_timings(e.h, 16, names, ms, launches)
    assert n > 0, lib.mpenv_last_error()
    out = {names[k].decode(): round(ms[k], 4) for k in range(n)}
    out["sum"] = round(sum(ms[k] for k in range(n)), 4)
    rc, info = R.scene_info(scene)
    assert rc == 0
    res = {"residency": "lds" if R.residency(e) == R.LDS else "global", "ms": out,
           "triangles": info.triangles, "collision_nodes": info.collision_nodes, "lidar_nodes": info.lidar_nodes,
           "collision_stack": info.collision_stack, "lidar_stack": info.lidar_stack,
           "global_bytes": info.global_bytes}
    e.mem.free(ring)
    e.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_residency_timing.json"))
    ap.add_argument("--worlds", type=int, default=16384)
    ap.add_argument("--team", type=int, default=6)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=100)
    args = ap.parse_args()
    result = {"workload": f"{args.team}v{args.team} x {args.worlds} worlds, device aim-bot over the hash tape, "
                          f"{args.warmup} warm-up + {args.steps} timed steps, ms per kernel per step",
              "configs": {}}
    with tempfile.TemporaryDirectory(prefix="mpenv_timing_") as tmp:
        p100 = big_scene.pillar_scene(os.path.join(tmp, "p100"), 100, 3)
        p400 = big_scene.pillar_scene(os.path.join(tmp, "p400"), 400, 3)
        for name, scene, mode in (("simple_map_lds", T.SCENE, R.LDS), ("simple_map_global", T.SCENE, R.GLOBAL),
                                  ("pillars_100_global", p100, None), ("pillars_400_global", p400, None)):
            result["configs"][name] = run(scene, mode, args.team, args.worlds, args.warmup, args.steps)
            print(name, json.dumps(result["configs"][name]["ms"]), file=sys.stderr, flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
