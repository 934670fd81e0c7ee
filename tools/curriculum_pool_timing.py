"""What the live curriculum pool costs (DESIGN.md §4 "k_harvest"), on the C3
batch, 6v6 x 16,384, in bench.py's driver window (run on the GPU box):

  parent      the parent commit's library (--parent-lib: its libmpenv.so,
              built from a checkout of that commit with build_native.py)
  off         this tree, no pool, no curriculum file
  file CAP    this tree, created with a curriculum_data_path file of CAP
              snapshots (the file is a pool row written by a short run)
  pool CAP    this tree, a pool of capacity CAP: in one process the window is
              timed at period 0 (nothing launched: the reset's reads of the
              pool alone, the same code path as `file`), 1, 16 and 64, ROUNDS
              times in turn; period p minus period 0 is what k_harvest adds to
              a step -- its launch and its device time on the step's stream

Each run is a fresh child process that loads one library (MPENV_LIB), replays
the captured step graph on one caller stream with bench.py's hash tape (a
64-step ring resident on the device, copied in before every step) and times
STEPS steps after WARMUP by two device events.  (parent, off) alternate PAIRS
times: the parent's min-max is the spread of this call and `off` is accepted
when its median lies inside it (exit status 1 otherwise).  Every other number
is a figure and gated on nothing.

usage: python tools/curriculum_pool_timing.py --parent-lib PATH [--out profiles/curriculum_pool_timing.json]
           [--worlds 16384] [--team 6] [--steps 1000] [--warmup 100] [--pairs 5] [--rounds 3]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

TAPE_SEED, RING = 1234, 64
CAPACITIES = (4096, 65536)
PERIODS = (0, 1, 16, 64)


def worker(args):
    """One run in this process: prints one JSON line."""
    import torch

    import mpenv_testlib as T

    mode, cap = args.worker, args.capacity
    W, ts = args.worlds, args.team
    path = None
    if mode == "file":
        # a pool row of a short run is a curriculum_data_path file
        import curriculum_testlib as CT

        e = T.Engine(W, ts)
        e.put_ctrl([0, 1, 1])
        e.init()
        assert CT.enable(e, CT.config(cap, period=1)) == 0, CT.err()
        for _ in range(8):
            e.step()
        path = os.path.join(tempfile.mkdtemp(prefix="mpenv_pool_"), "pool.bin")
        assert CT.MC.to_file(CT.read(e)[0], path) == cap
        e.close()
    e = T.Engine(W, ts, curriculum=path)
    A = e.W * e.N
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    ring = torch.from_numpy(T.mpenv_tape.tape_ring(TAPE_SEED, 0, A, RING)).cuda()
    e.put_ctrl([0, 1, 1])
    e.init()
    if mode == "pool":
        import curriculum_testlib as CT

        assert CT.enable(e, CT.config(cap, period=0)) == 0, CT.err()
    s = 0

    def steps(n):
        nonlocal s
        for _ in range(n):
            e._ok(e.lib.mpenv_copy_actions(e.h, ring.data_ptr() + (s % RING) * A * 24, st))
            e._ok(e.lib.mpenv_step_async(e.h, st))
            s += 1

    def timed(n):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        steps(n)
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1) / n

    steps(args.warmup)
    out = {"mode": mode, "capacity": cap}
    if mode == "pool":
        by = {p: [] for p in PERIODS}
        for _ in range(args.rounds):
            for p in PERIODS:
                assert CT.configure(e, CT.config(cap, period=p)) == 0, CT.err()
                steps(20)
                by[p].append(round(timed(args.steps), 4))
        out["ms_per_step_by_period"] = {str(p): v for p, v in by.items()}
        ticks = CT.read(e)[1]
        out["slots_written"] = int((ticks > 0).sum())
    else:
        out["ms_per_step"] = round(timed(args.steps), 4)
    out["graph_captures"] = e.graph_captures()
    e.close()
    print(json.dumps(out), flush=True)


def run(mode, lib, args, capacity=0):
    env = dict(os.environ)
    if lib:
        env["MPENV_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--capacity", str(capacity), "--worlds",
           str(args.worlds), "--team", str(args.team), "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--rounds", str(args.rounds)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(f"curriculum_pool_timing: the {mode} run failed with status {r.returncode}")
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(rec), file=sys.stderr, flush=True)
    return rec


def summary(ms):
    return {"ms_per_step": ms, "median": round(statistics.median(ms), 4), "min": min(ms), "max": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "curriculum_pool_timing.json"))
    ap.add_argument("--worlds", type=int, default=16384)
    ap.add_argument("--team", type=int, default=6)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--capacity", type=int, default=0)
    ap.add_argument("--worker", choices=["parent", "off", "file", "pool"], default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit("curriculum_pool_timing: --parent-lib must name the parent commit's libmpenv.so")
    parent_lib = os.path.abspath(args.parent_lib)
    runs = {"parent": [], "off": []}
    for _ in range(args.pairs):
        runs["parent"].append(run("parent", parent_lib, args))
        runs["off"].append(run("off", None, args))
    cfg = {k: summary([r["ms_per_step"] for r in v]) for k, v in runs.items()}
    inside = cfg["parent"]["min"] <= cfg["off"]["median"] <= cfg["parent"]["max"]
    pools = {}
    for cap in CAPACITIES:
        f = run("file", None, args, cap)
        p = run("pool", None, args, cap)
        med = {k: round(statistics.median(v), 4) for k, v in p["ms_per_step_by_period"].items()}
        pools[str(cap)] = {
            "file_ms_per_step": f["ms_per_step"],
            "pool_ms_per_step_by_period": p["ms_per_step_by_period"],
            "pool_median_by_period": med,
            "k_harvest_ms_by_period": {k: round(med[k] - med["0"], 4) for k in med if k != "0"},
            "k_harvest_share_of_step_by_period": {k: round((med[k] - med["0"]) / med["0"], 4) for k in med if k != "0"},
            "slots_written": p["slots_written"],
            "graph_captures": {"file": f["graph_captures"], "pool": p["graph_captures"]},
        }
    result = {
        "workload": f"{args.team}v{args.team} x {args.worlds} worlds, hash tape actions, captured step graph on one "
                    f"caller stream, fresh processes, {args.warmup} warm-up + {args.steps} timed steps per window",
        "configs": cfg,
        "off_inside_parent_spread": inside,
        "pools": pools,
    }
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    if not inside:
        raise SystemExit("curriculum_pool_timing: pool off lies outside the parent's spread in this call")


if __name__ == "__main__":
    main()
