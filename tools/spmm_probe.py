#!/usr/bin/env python3
"""Measurement harness: GrB_mxm with a FULL right operand — the spmm_full route (GRB_MI355X_FULL=1) beside the route the same call took before
(GRB_MI355X_FULL=0: the two-pass hash product), one process, operands in HBM only.

  --what sweep   A = R-MAT of scale 14 .. 20 (FP32 values), B full n x k for k in 1, 4, 16, 64, 256, FP32 PLUS_TIMES.  Five timed calls of each route after a warm-up;
                 `noise_ms` is the larger spread (max - min) of the two, `full_over_hash` the ratio of the medians, `slower_beyond_noise` whether the new route lost
                 by more than the noise.  The smallest nnz(A) k from which the new route never loses is the threshold (SPMM_FULL_MIN_PRODUCTS).  The old route is not
                 run beyond --max-hash-products products (it expands every one of them).
  --what big     R-MAT 20 and 22, k = 16 and 64, beside a device copy of the algorithmic bytes (A's columns and values, nnz k gathered values, T's values and
                 columns: `copy_ms` moves that many bytes, half read and half written) — `over_copy` is the route's time over it; FP64 PLUS_TIMES and FP32 MIN_PLUS at
                 scale 20; and the share of T.col: `pattern_ms` is the fill of a row pointer and nnz(T) column words alone (Matrix.from_dense of T's shape minus a copy
                 of its values), `col_share` its part of the product's time — what a column-free full format would save.
Whole-call HIP-event times.  Every step runs under --step-seconds (SIGALRM) and the probe stops at the first failure.  One JSON line per measurement is appended to
--out (default profiles/spmm_full_probe.jsonl).  Run each --what as its own command under `timeout`."""
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
            sys.exit(f"spmm_probe.py: step '{self.what}' passed its limit of {self.seconds} s")
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


def routed(gb, hook, call, reps):
    os.environ["GRB_MI355X_FULL"] = hook
    try:
        t, plan = runs(gb, call, reps)
    finally:
        del os.environ["GRB_MI355X_FULL"]
    assert plan.startswith("spmm_full<") == (hook == "1"), (hook, plan)
    return t, plan


def torch_dtype(typ):
    import torch
    return {np.float32: torch.float32, np.float64: torch.float64}[typ._np]


def left_operand(gb, scale, typ, seed=42):
    """(A, nnz, non-empty rows): the R-MAT matrix with uniform values, in HBM only."""
    from pygraphblas_amd import rmat
    n = 1 << scale
    rp, col = rmat.csr_numpy(scale, seed=seed)
    rng = np.random.default_rng(seed)
    A = gb.Matrix.from_csr(typ, n, n, rp.astype(np.uint32), col.astype(np.uint32), rng.random(len(col)).astype(typ._np))
    return A, int(len(col)), int((np.diff(rp) > 0).sum())


def full_operand(gb, n, k, typ):
    import torch
    return gb.Matrix.from_dense(torch.rand((n, k), dtype=torch_dtype(typ), device="cuda"))


def sweep(args):
    import pygraphblas_amd as gb
    T = gb.FP32
    for scale in range(args.min_scale, args.max_scale + 1):
        with step(args.step_seconds, f"operand A {scale}"):
            A, nnz, nonempty = left_operand(gb, scale, T)
        for k in (1, 4, 16, 64, 256):
            with step(args.step_seconds, f"operand H {scale} {k}"):
                H = full_operand(gb, 1 << scale, k, T)
            rec = {"probe": "sweep", "scale": scale, "k": k, "type": "FP32", "semiring": "PLUS_TIMES", "nnz_a": nnz, "products": nnz * k, "nvals_t": nonempty * k}
            with step(args.step_seconds, "full"):
                f, plan = routed(gb, "1", lambda: A.mxm(H, semiring=T.PLUS_TIMES), args.reps)
            rec.update(full_runs_ms=f, full_ms=float(np.median(f)), full_plan=plan)
            if nnz * k <= args.max_hash_products:
                with step(args.step_seconds, "hash"):
                    h, hplan = routed(gb, "0", lambda: A.mxm(H, semiring=T.PLUS_TIMES), args.reps)
                rec.update(hash_runs_ms=h, hash_ms=float(np.median(h)), hash_plan=hplan[:120], noise_ms=round(max(max(f) - min(f), max(h) - min(h)), 4))
                rec["full_over_hash"] = round(rec["full_ms"] / rec["hash_ms"], 4)
                rec["slower_beyond_noise"] = rec["full_ms"] - rec["hash_ms"] > rec["noise_ms"]
            else:
                rec["hash_ms"] = None                                             # not run: beyond --max-hash-products
            emit(args.out, rec)
            del H
        del A


def copy_ms(nbytes, reps):
    """Median time of a device copy that moves `nbytes` in all (half read, half written)."""
    import torch
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
    times = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); a.record(); dst.copy_(src); b.record(); torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times[1:]))


def big(args):
    import torch
    import pygraphblas_amd as gb
    for scale, k, T, sr in ((20, 16, gb.FP32, "PLUS_TIMES"), (20, 64, gb.FP32, "PLUS_TIMES"), (20, 64, gb.FP64, "PLUS_TIMES"), (20, 64, gb.FP32, "MIN_PLUS"),
                            (22, 16, gb.FP32, "PLUS_TIMES"), (22, 64, gb.FP32, "PLUS_TIMES")):
        if scale > args.max_scale:
            continue
        with step(args.step_seconds, f"operands {scale} {k}"):
            A, nnz, nonempty = left_operand(gb, scale, T); H = full_operand(gb, 1 << scale, k, T)
        ts = np.dtype(T._np).itemsize; nt = nonempty * k
        nbytes = nnz * (4 + ts) + nnz * k * ts + nt * (ts + 4)
        rec = {"probe": "big", "scale": scale, "k": k, "type": T.__name__, "semiring": sr, "nnz_a": nnz, "products": nnz * k, "nvals_t": nt, "algorithmic_bytes": nbytes}
        with step(args.step_seconds, "full"):
            f, plan = routed(gb, "1", lambda: A.mxm(H, semiring=getattr(T, sr)), args.reps)
        with step(args.step_seconds, "copy"):
            c = copy_ms(nbytes, args.reps)
        rec.update(full_runs_ms=f, full_ms=float(np.median(f)), full_plan=plan, copy_ms=round(c, 4), over_copy=round(float(np.median(f)) / c, 3),
                   algorithmic_gb_per_s=round(nbytes / float(np.median(f)) / 1e6, 1))
        with step(args.step_seconds, "pattern"):
            X = torch.empty((nonempty, k), dtype=torch_dtype(T), device="cuda")
            imp, _ = runs(gb, lambda: gb.Matrix.from_dense(X), args.reps)
            vals = copy_ms(2 * nt * ts, args.reps)
        rec.update(import_full_ms=float(np.median(imp)), value_copy_ms=round(vals, 4), pattern_ms=round(max(float(np.median(imp)) - vals, 0.0), 4))
        rec["col_share"] = round(rec["pattern_ms"] / rec["full_ms"], 3)
        emit(args.out, rec)
        del A, H, X


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["sweep", "big"], required=True)
    ap.add_argument("--min-scale", type=int, default=14)
    ap.add_argument("--max-scale", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-hash-products", type=int, default=1 << 30)
    ap.add_argument("--step-seconds", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spmm_full_probe.jsonl"))
    args = ap.parse_args()
    if args.max_scale is None:
        args.max_scale = 20 if args.what == "sweep" else 22
    {"sweep": sweep, "big": big}[args.what](args)
