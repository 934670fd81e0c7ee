"""What the league scheduler costs (DESIGN.md §4 "League scheduling"), on the C3
batch, 6v6 x 16,384, in bench.py's driver window (run on the GPU box):

  parent   the parent commit's library (--parent-lib: its libmpenv.so, built
           from a checkout of that commit with build_native.py)
  off      this tree, no league enabled
  on       this tree, league enabled: MPENV_LEAGUE_DRAW_TEAM1, P = 8

Each run is a fresh child process that loads one library (MPENV_LIB), replays
the captured step graph on one caller stream with bench.py's hash tape (a
64-step ring resident on the device, copied in before every step) and times
STEPS steps after WARMUP by two device events.  The runs alternate in pairs --
(parent, off), (parent, on), ... -- PAIRS times each, so the parent is timed
twice as often as either of the others: its min-max over those runs is the
spread of this call, and `off` is accepted when its median lies inside it
(exit status 1 otherwise).  `on` is a figure and gated on nothing.

The off and on runs also time, after the window, single steps by a pair of
events each: 20 ordinary ones, and 5 in which every world ends (every RESET
row set in front of the step) -- the contention case: 16,384 episodes in one
launch into the eight cells of home id 0 (team 0 is never re-drawn, team 1 is
drawn from row 0's uniform weights).  on - off of that figure is what
k_league adds to such a step.

usage: python tools/league_timing.py --parent-lib PATH [--out profiles/league_timing.json]
           [--worlds 16384] [--team 6] [--steps 1000] [--warmup 100] [--pairs 3]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

TAPE_SEED, RING = 1234, 64
LEAGUE_P = 8


def worker(args):
    """One run in this process: prints one JSON line."""
    import numpy as np
    import torch

    import mpenv_testlib as T

    mode = args.worker
    W, ts = args.worlds, args.team
    e = T.Engine(W, ts)
    A = e.W * e.N
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    ring = torch.from_numpy(T.mpenv_tape.tape_ring(TAPE_SEED, 0, A, RING)).cuda()
    e.put_ctrl([0, 1, 1])
    if mode == "on":
        import league_testlib as L

        assert L.enable(e, L.config(LEAGUE_P, L.TEAM1, 1)) == 0, L.err()
    e.init()
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
    out = {"mode": mode, "ms_per_step": round(timed(args.steps), 4)}
    if mode != "parent":
        out["single_step_ms"] = round(statistics.median(timed(1) for _ in range(20)), 4)
        ones = np.ones((W, 1), np.int32)
        mass = []
        for _ in range(5):
            steps(3)
            stream.synchronize()
            e.put("RESET", ones)
            mass.append(timed(1))
        out["all_worlds_end_step_ms"] = [round(v, 4) for v in mass]
        if mode == "on":
            table = L.read(e, L.TABLE)
            out["episodes_recorded"] = int(table[..., 0].sum())
            out["draws_min_max"] = [int(v) for v in (L.read(e, L.DRAWS).min(), L.read(e, L.DRAWS).max())]
    out["graph_captures"] = e.graph_captures()
    e.close()
    print(json.dumps(out), flush=True)


def run(mode, lib, args):
    env = dict(os.environ)
    if lib:
        env["MPENV_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--worlds", str(args.worlds), "--team",
           str(args.team), "--steps", str(args.steps), "--warmup", str(args.warmup)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(f"league_timing: the {mode} run failed with status {r.returncode}")
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(rec), file=sys.stderr, flush=True)
    return rec


def summary(ms):
    return {"ms_per_step": ms, "median": round(statistics.median(ms), 4), "min": min(ms), "max": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "league_timing.json"))
    ap.add_argument("--worlds", type=int, default=16384)
    ap.add_argument("--team", type=int, default=6)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--worker", choices=["parent", "off", "on"], default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit("league_timing: --parent-lib must name the parent commit's libmpenv.so")
    if args.pairs < 3:
        raise SystemExit("league_timing: at least three pairs")
    parent_lib = os.path.abspath(args.parent_lib)
    runs = {"parent": [], "off": [], "on": []}
    for _ in range(args.pairs):
        for other in ("off", "on"):
            runs["parent"].append(run("parent", parent_lib, args))
            runs[other].append(run(other, None, args))
    cfg = {k: summary([r["ms_per_step"] for r in v]) for k, v in runs.items()}
    inside = cfg["parent"]["min"] <= cfg["off"]["median"] <= cfg["parent"]["max"]
    med = lambda rs, key: round(statistics.median(x for r in rs for x in (r[key] if isinstance(r[key], list) else [r[key]])), 4)  # noqa: E731
    result = {
        "workload": f"{args.team}v{args.team} x {args.worlds} worlds, hash tape actions, captured step graph on one "
                    f"caller stream, {args.pairs} alternating pairs of fresh processes per comparison, "
                    f"{args.warmup} warm-up + {args.steps} timed steps each",
        "league": f"MPENV_LEAGUE_DRAW_TEAM1, P = {LEAGUE_P}",
        "configs": cfg,
        "off_inside_parent_spread": inside,
        "on_minus_off_ms_per_step": round(cfg["on"]["median"] - cfg["off"]["median"], 4),
        "single_step_ms": {k: med(runs[k], "single_step_ms") for k in ("off", "on")},
        "all_worlds_end_step_ms": {k: med(runs[k], "all_worlds_end_step_ms") for k in ("off", "on")},
        "all_worlds_end_step_runs": {k: [r["all_worlds_end_step_ms"] for r in runs[k]] for k in ("off", "on")},
        "episodes_recorded": [r["episodes_recorded"] for r in runs["on"]],
        "draws_min_max": [r["draws_min_max"] for r in runs["on"]],
        "graph_captures": {k: [r["graph_captures"] for r in v] for k, v in runs.items()},
    }
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    if not inside:
        raise SystemExit("league_timing: league off lies outside the parent's spread in this call")


if __name__ == "__main__":
    main()
