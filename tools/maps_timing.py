"""What a map set's per-range launches cost (DESIGN.md §4 "Map sets"), on the
C3 batch, 6v6 x 16,384 (run on the GPU box):

  single        a single-map manager on scenes/simple_map (mpenv_create)
  sets_M        a map set of M equal ranges, M in 1, 2, 4, 8, 16, 32, all on
                scenes/simple_map: the same work and the same results, 5 M
                kernels in the captured step graph instead of 5
  mixed         [simple_map, "blocks"] at 8,192 worlds each (tests/maps_testlib.py
                map B, global-resident) against single-map managers on each

Every manager replays its captured step graph on one caller stream; the
actions are bench.py's hash tape (64-step ring resident on the device, copied
in before every step).  A round times STEPS steps after WARMUP by two device
events around them, one manager after the other; ROUNDS rounds alternate the
managers, and a figure is the median (min-max) of the rounds' ms per step.

usage: python tools/maps_timing.py [--out profiles/maps_timing.json] [--worlds 16384] [--team 6]
                                   [--steps 1000] [--warmup 100] [--rounds 5]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import maps_testlib as M  # noqa: E402
import mpenv_testlib as T  # noqa: E402

TAPE_SEED, RING = 1234, 64


class Timed:
    def __init__(self, e, stream):
        import torch

        self.e, self.stream, self.s = e, stream, 0
        A = e.W * e.N
        self.A = A
        self.ring = torch.from_numpy(T.mpenv_tape.tape_ring(TAPE_SEED, 0, A, RING)).cuda()
        e.put_ctrl([0, 1, 1])
        e.init()

    def steps(self, n):
        e, st = self.e, self.stream.cuda_stream
        for _ in range(n):
            src = self.ring.data_ptr() + (self.s % RING) * self.A * 24
            e._ok(e.lib.mpenv_copy_actions(e.h, src, st))
            e._ok(e.lib.mpenv_step_async(e.h, st))
            self.s += 1

    def round(self, warmup, steps):
        import torch

        self.steps(warmup)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(self.stream)
        self.steps(steps)
        t1.record(self.stream)
        t1.synchronize()
        return t0.elapsed_time(t1) / steps


def summary(ms):
    return {"ms_per_step": [round(v, 4) for v in ms], "median": round(statistics.median(ms), 4),
            "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maps_timing.json"))
    ap.add_argument("--worlds", type=int, default=16384)
    ap.add_argument("--team", type=int, default=6)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    W, ts = args.worlds, args.team
    stream = torch.cuda.Stream()
    A, B = M.scene("A"), M.scene("B")
    runs = {"single": Timed(T.Engine(W, ts), stream)}
    for m in (1, 2, 4, 8, 16, 32):
        runs[f"sets_{m}"] = Timed(M.MapEngine([(A, W // m)] * m, ts), stream)
    runs["mixed_A_B"] = Timed(M.MapEngine([(A, W // 2), (B, W // 2)], ts), stream)
    runs["single_B"] = Timed(T.Engine(W, ts, scene=B), stream)
    ms = {k: [] for k in runs}
    for r in range(args.rounds):
        for k, run in runs.items():
            ms[k].append(run.round(args.warmup, args.steps))
            print(f"round {r} {k} {ms[k][-1]:.4f}", file=sys.stderr, flush=True)
    result = {"workload": f"{ts}v{ts} x {W} worlds, hash tape actions, captured step graph on one caller stream, "
                          f"{args.rounds} alternating rounds of {args.warmup} warm-up + {args.steps} timed steps",
              "graph_captures": {k: run.e.graph_captures() for k, run in runs.items()},
              "configs": {k: summary(v) for k, v in ms.items()}}
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
