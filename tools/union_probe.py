#!/usr/bin/env python3
"""Measurement harness: GxB_eWiseUnion beside eWiseAdd on the same operands, one process, operands in HBM only.

  --what matrix   two R-MAT matrices (--scale, default 20; seeds 42 and 43) FP64: `A.eunion(B, MINUS, 0, 0)`, the plain `A.eadd(B, PLUS)`, and what the union
                  replaces — a pattern union, two masked scalar assigns and an eadd (`emulated`: zeros on the pattern union, A and B laid over them, then emult MINUS: five calls).
  --what vector   two FP32 vectors of 2^--log2n (default 26) positions at 50 % density: union and eadd, without an accumulator (k_vec_ewise) and with one (the
                  one-pass kernel), in blocking mode — a lone eadd would otherwise be queued.
The claim to check is "the union is within the run-to-run noise of eadd": `eadd_runs_ms` holds five timed eadd calls, `noise_ms` their spread (max - min), and
`union_minus_eadd_ms` the difference of the medians.  Whole-call HIP-event times, --reps calls after a warm-up.  Every step runs under --step-seconds (SIGALRM)
and the probe stops at the first failure.  One JSON line per measurement is appended to --out (default profiles/union_probe.jsonl).  Run each --what as its own
command under `timeout`."""
import argparse
import ctypes as C
import json
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def emit(out, rec):
    print(json.dumps(rec), flush=True)
    with open(out, "a") as f:
        f.write(json.dumps(rec) + "\n")


class step:
    """A time limit for one step: the probe ends there (nothing more is started on the GPU)."""
    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def __enter__(self):
        def over(signum, frame):
            sys.exit(f"union_probe.py: step '{self.what}' passed its limit of {self.seconds} s")
        signal.signal(signal.SIGALRM, over)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def runs(gb, call, reps):
    """Event times of `reps` calls after one warm-up, and the plan string of the last."""
    times = []
    for _ in range(reps + 1):
        gb.lib.GrBX_device_synchronize()
        gb.lib.GrBX_timer_start()
        out = call()
        ms = C.c_float(0)
        gb.lib.GrBX_timer_stop(C.byref(ms))
        plan = gb.last_kernel_plan()
        del out
        times.append(round(ms.value, 4))
    return times[1:], plan


def compare(gb, args, rec, union, eadd, emulated):
    with step(args.step_seconds, "eadd"):
        e, _ = runs(gb, eadd, 5)
    with step(args.step_seconds, "union"):
        u, plan = runs(gb, union, args.reps)
    rec.update(eadd_runs_ms=e, eadd_ms=float(np.median(e)), noise_ms=round(max(e) - min(e), 4), union_ms=float(np.median(u)), union_plan=plan)
    rec["union_minus_eadd_ms"] = round(rec["union_ms"] - rec["eadd_ms"], 4)
    rec["within_noise"] = abs(rec["union_minus_eadd_ms"]) <= rec["noise_ms"]
    if emulated:
        with step(args.step_seconds, "emulated"):
            m, _ = runs(gb, emulated, args.reps)
        rec["emulated_ms"] = float(np.median(m)); rec["emulated_over_union"] = round(rec["emulated_ms"] / rec["union_ms"], 2)
    emit(args.out, rec)


def matrix(args):
    import pygraphblas_amd as gb
    from pygraphblas_amd import rmat
    n = 1 << args.scale; T = gb.FP64; ops = []
    for seed in (42, 43):
        rp, col = rmat.csr_numpy(args.scale, seed=seed)
        vals = np.random.default_rng(seed).standard_normal(len(col))
        ops.append(gb.Matrix.from_csr(T, n, n, rp.astype(np.uint32), col.astype(np.uint32), vals))      # HBM only
    A, B = ops

    def emulated():                                                             # five calls, four merges of the two patterns
        zeros = A.eadd(B, T.PLUS).apply_second(T.TIMES, 0.0)                    # the pattern union, holding 0
        Ap = zeros.eadd(A, T.SECOND); Bp = zeros.eadd(B, T.SECOND)              # A / B over it: 0 where the other alone has the entry
        return Ap.emult(Bp, T.MINUS)
    rec = {"probe": "matrix", "scale": args.scale, "type": "FP64", "entries_a": int(A.nvals), "entries_b": int(B.nvals)}
    compare(gb, args, rec, lambda: A.eunion(B, T.MINUS, 0, 0), lambda: A.eadd(B, T.PLUS), emulated)


def vector(args):
    os.environ.setdefault("GRB_MI355X_BLOCKING", "1")                           # a lone eadd would be queued, and its call would time the queueing
    import pygraphblas_amd as gb
    n = 1 << args.log2n; T = gb.FP32; rng = np.random.default_rng(7)
    mk = lambda: gb.Vector.from_dense_array(rng.standard_normal(n).astype(np.float32), T, present=(rng.random(n) < 0.5).view(np.uint8))
    u, v, w = mk(), mk(), mk()
    for accum in (None, T.PLUS):
        out = w if accum else None
        rec = {"probe": "vector", "n": n, "type": "FP32", "density": 0.5, "accum": bool(accum)}
        compare(gb, args, rec, lambda: u.eunion(v, T.MINUS, 0, 0, out=out, accum=accum), lambda: u.eadd(v, T.PLUS, out=out, accum=accum), None)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["matrix", "vector"], required=True)
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--log2n", type=int, default=26)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-seconds", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "union_probe.jsonl"))
    args = ap.parse_args()
    {"matrix": matrix, "vector": vector}[args.what](args)
