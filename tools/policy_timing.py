"""Times in-sim policy inference (csrc/policy.hip) on the C3 batch, 6v6 x
16,384, and the C2 batch, 3v3 x 4,096 (run on the GPU box): the policy part of
a step (selection, embed kernel, trunk kernel; mpenv_debug_policy_step) with
100 %, 50 % (one team) and 10 % of the agents on the policy, the embed and
trunk kernels apart at 100 %, and mpenv_policy_forward.

HIP events on one stream around REPS back-to-back calls, the variants
interleaved over ROUNDS rounds (after a warm-up round); each figure is the
median round, with the fastest and slowest beside it.  The floor is
arithmetic: 801,536 multiply-adds per agent at the 155 TF/s measured for the
f32-input MFMA; trunk_tflops counts the trunk's and heads' 739,840
multiply-adds per agent over the trunk kernel's time.  The checkpoint is the
random one of tests/policy_testlib.py (the time does not depend on the values).

--precision f32 | bf16 | both (mpenv_policy_precision.h): which trunk kernel
runs.  With both, the two precisions alternate round by round inside the one
run, on the same manager and the same observations, and the result holds one
block per precision and the bf16 / f32 ratio of every call's median.

--slots N (league play, mpenv_policy_slots.h): N synthetic checkpoints in
slots 0 .. N-1 and the policy agents dealt over them evenly, agent by agent;
mpenv_policy_forward stays slot 0 for every agent.  --batches picks C3, C2 or
both.

usage: python tools/policy_timing.py [--slots N] [--batches C3,C2] [--precision f32|bf16|both]
                                     [--out profiles/policy_timing.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mpenv_testlib as T  # noqa: E402
import policy_bf16_testlib as B  # noqa: E402
import policy_slots_abi  # noqa: E402
import policy_testlib as P  # noqa: E402

REPS, ROUNDS = 3, 5
MACS_TOTAL = 801536
MACS_TRUNK = 384 * 512 + 2 * 512 * 512 + 512 * 37
PEAK_TFLOPS = 155.0
BF16_RATE = 16  # v_mfma_f32_32x32x16_bf16 over v_mfma_f32_32x32x2_f32, multiply-adds per cycle
PRECISIONS = {"f32": B.F32, "bf16": B.BF16}
SELECT, EMBED, TRUNK, ALL = 1, 2, 4, 7


def measure(ts, W, ckpts, precisions):
    """{precision: result} for the precisions named, alternating round by round"""
    A = W * 2 * ts
    lib = B.bind(T.lib_mpenv())
    e = T.Engine(W, ts)
    hip = e.mem.hip
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]

    def ok(rc):
        assert rc == 0, (rc, lib.mpenv_last_error())

    st, ev0, ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(hip.hipStreamCreate(C.byref(st)))
    ok(hip.hipEventCreate(C.byref(ev0)))
    ok(hip.hipEventCreate(C.byref(ev1)))

    # observations worth reading: 20 steps of the seek-and-fight action source
    e.put_ctrl([0, 1, 1])
    e.init()
    ring = e.mem.upload(T.mpenv_tape.tape_ring(1234, 0, A, 4))
    for s in range(20):
        e.combat_actions(ring + (s % 4) * A * 24, None, 1)
        e.step()
    if len(ckpts) == 1:
        ok(lib.mpenv_policy_load(e.h, ckpts[0].encode()))
    else:
        policy_slots_abi.bind(lib)
        for slot, ckpt in enumerate(ckpts):
            ok(lib.mpenv_policy_load_slot(e.h, slot, ckpt.encode()))

    rng = np.random.default_rng(3)
    team0 = (np.arange(A) % (2 * ts)) < ts
    ids = {"100pct": np.zeros(A, np.int32), "50pct_one_team": np.where(team0, 0, -2).astype(np.int32),
           "10pct": np.where(rng.uniform(0, 1, A) < 0.1, 0, -2).astype(np.int32)}
    for v in ids.values():  # the k-th policy agent on checkpoint k mod N
        on = np.flatnonzero(v >= 0)
        v[on] = np.arange(len(on)) % len(ckpts)
    logits = e.mem.upload(np.zeros((A, P.LOGITS), np.float32))
    variants = [(f"step_policy_{k}", k, ALL) for k in ids]
    variants += [("select_embed_100pct", "100pct", SELECT | EMBED), ("trunk_100pct", "100pct", TRUNK),
                 ("forward_100pct", "100pct", 0)]
    times = {prec: {name: [] for name, _, _ in variants} for prec in precisions}
    for rnd in range(ROUNDS + 1):
        for prec in precisions:
            ok(lib.mpenv_policy_set_precision(e.h, PRECISIONS[prec]))
            for name, which, parts in variants:
                e.put("AGENT_POLICY", ids[which])
                ok(lib.mpenv_debug_policy_step(e.h, ALL, st))  # the list and the embeddings of this variant
                ok(hip.hipEventRecord(ev0, st))
                for _ in range(REPS):
                    if parts:
                        ok(lib.mpenv_debug_policy_step(e.h, parts, st))
                    else:
                        ok(lib.mpenv_policy_forward(e.h, logits, None, st))
                ok(hip.hipEventRecord(ev1, st))
                ok(hip.hipEventSynchronize(ev1))
                ms = C.c_float()
                ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1))
                if rnd > 0:  # round 0 warms every variant up
                    times[prec][name].append(ms.value / REPS)
    # the floor: the embed kernel's multiply-adds at the f32 rate, the trunk's at the precision's
    results = {}
    for prec in precisions:
        rate = PEAK_TFLOPS * 1e12 * (BF16_RATE if prec == "bf16" else 1)
        floor_ms = A * 2 * ((MACS_TOTAL - MACS_TRUNK) / (PEAK_TFLOPS * 1e12) + MACS_TRUNK / rate) * 1e3
        out = {"workload": f"{ts}v{ts} x {W} worlds ({A} agents) after 20 seek-and-fight steps",
               "precision": prec, "checkpoint_slots": len(ckpts),
               "floor_ms_all_agents": round(floor_ms, 4), "reps_per_round": REPS, "rounds": ROUNDS, "calls": {}}
        for name, which, _ in variants:
            t = times[prec][name]
            ms = statistics.median(t)
            n = int((ids[which] >= 0).sum())
            out["calls"][name] = {"ms": round(ms, 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                                  "policy_agents": n, "us_per_1000_agents": round(ms * 1e3 / n * 1e3, 3)}
        full = out["calls"]["step_policy_100pct"]["ms"]
        out["step_policy_100pct_over_floor"] = round(full / floor_ms, 3)
        out["trunk_tflops"] = round(A * MACS_TRUNK * 2 / (out["calls"]["trunk_100pct"]["ms"] * 1e-3) / 1e12, 2)
        out["embed_share_of_call"] = round(out["calls"]["select_embed_100pct"]["ms"] / full, 3)
        results[prec] = out
    e.mem.free(logits)
    e.mem.free(ring)
    e.close()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_timing.json"))
    ap.add_argument("--slots", type=int, default=1, help="checkpoints, in slots 0 .. N-1 (1 to 32)")
    ap.add_argument("--batches", default="C3,C2")
    ap.add_argument("--precision", choices=["f32", "bf16", "both"], default="f32")
    args = ap.parse_args()
    if not 1 <= args.slots <= policy_slots_abi.POLICY_SLOTS:
        ap.error("--slots must be in [1, 32]")
    shapes = {"C3": (6, 16384), "C2": (3, 4096)}
    with tempfile.TemporaryDirectory() as d:
        ckpts = [os.path.join(d, f"ckpt{k}") for k in range(args.slots)]
        for k, ckpt in enumerate(ckpts):
            P.write_checkpoint(ckpt, 21 + k)
        precisions = ["f32", "bf16"] if args.precision == "both" else [args.precision]
        out = {}
        for b in args.batches.split(","):
            res = measure(*shapes[b], ckpts, precisions)
            if len(precisions) == 1:
                out[b] = res[precisions[0]]
                continue
            res["bf16_over_f32"] = {name: round(res["bf16"]["calls"][name]["ms"] / res["f32"]["calls"][name]["ms"], 3)
                                    for name in res["f32"]["calls"]}
            out[b] = res
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
