#!/usr/bin/env python3
"""Measurement harness: GrB_mxm of two FULL matrices under a plain mask, S<M> = X (+).(x) Y' — the sddmm route (GRB_MI355X_SDDMM=1) beside the route the same
call took before (GRB_MI355X_SDDMM=0: the masked Gustavson product over CSR operands and Y's materialised transpose), one process, operands in HBM only.

  --what sweep   m = n = 2^8 .. 2^12, uniform masks of 1, 4, 16, 64 entries per row, k in 1, 4, 16, 64, 256, FP32 PLUS_TIMES, the call `M.sddmm(X, Y)`.  Five timed
                 calls of each route after a warm-up; `noise_ms` is the larger spread (max - min) of the two, `sddmm_over_masked` the ratio of the medians,
                 `slower_beyond_noise` whether the new route lost by more than the noise.  The smallest work count m k n from which the new route never loses is
                 the threshold (SDDMM_MIN_WORK).  The old route is not run beyond --max-masked-work probes (it makes every one of them).
  --what big     R-MAT 18 and 20 as the mask, k = 16, 64, 256, FP32 and FP64, MIN_PLUS, beside a device copy of the algorithmic bytes
                 (nnz (2 k size + 4 + size): both rows of every entry, its column, its result — `copy_ms` moves that many bytes, half read and half written;
                 `over_copy` is the route's time over it) and beside spmm_full on the same (A, k): `A.mxm(H)` with H full n x k (GRB_MI355X_FULL=1).
Whole-call HIP-event times.  Every step runs under --step-seconds (SIGALRM) and the probe stops at the first failure.  One JSON line per measurement is appended to
--out (default profiles/sddmm_probe.jsonl).  Run each --what as its own command under `timeout`."""
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
            sys.exit(f"sddmm_probe.py: step '{self.what}' passed its limit of {self.seconds} s")
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


def routed(gb, name, hook, prefix, call, reps):
    os.environ[name] = hook
    try:
        t, plan = runs(gb, call, reps)
    finally:
        del os.environ[name]
    assert plan.startswith(prefix) == (hook == "1"), (name, hook, plan)
    return t, plan


def torch_dtype(typ):
    import torch
    return {np.float32: torch.float32, np.float64: torch.float64}[typ._np]


def full_operand(gb, n, k, typ):
    import torch
    return gb.Matrix.from_dense(torch.rand((n, k), dtype=torch_dtype(typ), device="cuda"))


def uniform_mask(gb, m, n, per_row, seed):
    """`per_row` entries in every row, evenly spaced from a random first column: BOOL, in HBM only."""
    rng = np.random.default_rng(seed)
    cols = np.sort((rng.integers(0, n, (m, 1)) + np.arange(per_row)[None, :] * (n // per_row)) % n, axis=1)
    rp = np.arange(m + 1, dtype=np.uint32) * np.uint32(per_row)
    return gb.Matrix.from_csr(gb.BOOL, m, n, rp, cols.ravel().astype(np.uint32), np.ones(m * per_row, np.bool_))


def sweep(args):
    import pygraphblas_amd as gb
    T = gb.FP32
    for scale in range(args.min_scale, args.max_scale + 1):
        n = 1 << scale
        for per_row in (1, 4, 16, 64):
            with step(args.step_seconds, f"mask {scale} {per_row}"):
                M = uniform_mask(gb, n, n, per_row, seed=scale * 100 + per_row)
            for k in (1, 4, 16, 64, 256):
                with step(args.step_seconds, f"operands {scale} {k}"):
                    X = full_operand(gb, n, k, T); Y = full_operand(gb, n, k, T)
                work = n * k * n
                rec = {"probe": "sweep", "m": n, "n": n, "per_row": per_row, "k": k, "type": "FP32", "semiring": "PLUS_TIMES", "entries": n * per_row, "products": n * per_row * k, "masked_work": work}
                call = lambda: M.sddmm(X, Y, T.PLUS_TIMES)
                with step(args.step_seconds, "sddmm"):
                    f, plan = routed(gb, "GRB_MI355X_SDDMM", "1", "sddmm<", call, args.reps)
                rec.update(sddmm_runs_ms=f, sddmm_ms=float(np.median(f)), sddmm_plan=plan)
                if work <= args.max_masked_work:
                    with step(args.step_seconds, "masked"):
                        h, hplan = routed(gb, "GRB_MI355X_SDDMM", "0", "sddmm<", call, args.reps)
                    rec.update(masked_runs_ms=h, masked_ms=float(np.median(h)), masked_plan=hplan[:120], noise_ms=round(max(max(f) - min(f), max(h) - min(h)), 4))
                    rec["sddmm_over_masked"] = round(rec["sddmm_ms"] / rec["masked_ms"], 4)
                    rec["slower_beyond_noise"] = rec["sddmm_ms"] - rec["masked_ms"] > rec["noise_ms"]
                else:
                    rec["masked_ms"] = None                                         # not run: beyond --max-masked-work
                emit(args.out, rec)
                del X, Y
            del M


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
    import pygraphblas_amd as gb
    from pygraphblas_amd import rmat
    for scale in (18, 20):
        if scale > args.max_scale:
            continue
        n = 1 << scale
        with step(args.step_seconds, f"mask {scale}"):
            rp, col = rmat.csr_numpy(scale, seed=42)
            rp32, col32 = rp.astype(np.uint32), col.astype(np.uint32); nnz = int(len(col))
            M = gb.Matrix.from_csr(gb.BOOL, n, n, rp32, col32, np.ones(nnz, np.bool_))
        for T in (gb.FP32, gb.FP64):
            ts = np.dtype(T._np).itemsize
            with step(args.step_seconds, f"A {scale}"):
                A = gb.Matrix.from_csr(T, n, n, rp32, col32, np.random.default_rng(1).random(nnz).astype(T._np))
            for k in (16, 64, 256):
                with step(args.step_seconds, f"operands {scale} {k}"):
                    X = full_operand(gb, n, k, T); Y = full_operand(gb, n, k, T)
                nbytes = nnz * (2 * k * ts + 4 + ts)
                rec = {"probe": "big", "scale": scale, "k": k, "type": T.__name__, "semiring": "MIN_PLUS", "entries": nnz, "products": nnz * k, "algorithmic_bytes": nbytes}
                with step(args.step_seconds, "sddmm"):
                    f, plan = routed(gb, "GRB_MI355X_SDDMM", "1", "sddmm<", lambda: M.sddmm(X, Y, T.MIN_PLUS), args.reps)
                with step(args.step_seconds, "copy"):
                    c = copy_ms(nbytes, args.reps)
                with step(args.step_seconds, "spmm_full"):
                    s, splan = routed(gb, "GRB_MI355X_FULL", "1", "spmm_full<", lambda: A.mxm(Y, semiring=T.MIN_PLUS), args.reps)
                rec.update(sddmm_runs_ms=f, sddmm_ms=float(np.median(f)), sddmm_plan=plan, copy_ms=round(c, 4), over_copy=round(float(np.median(f)) / c, 3),
                           algorithmic_gb_per_s=round(nbytes / float(np.median(f)) / 1e6, 1), spmm_full_runs_ms=s, spmm_full_ms=float(np.median(s)), spmm_full_plan=splan,
                           sddmm_over_spmm_full=round(float(np.median(f)) / float(np.median(s)), 3))
                emit(args.out, rec)
                del X, Y
            del A
        del M


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["sweep", "big"], required=True)
    ap.add_argument("--min-scale", type=int, default=None)
    ap.add_argument("--max-scale", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-masked-work", type=int, default=1 << 33)
    ap.add_argument("--step-seconds", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sddmm_probe.jsonl"))
    args = ap.parse_args()
    if args.min_scale is None:
        args.min_scale = 8
    if args.max_scale is None:
        args.max_scale = 12 if args.what == "sweep" else 20
    {"sweep": sweep, "big": big}[args.what](args)
