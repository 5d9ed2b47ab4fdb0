#!/usr/bin/env python3
"""Measurement harness: GrB_mxv / GrB_vxm with a FULL matrix — the gemv_full route (GRB_MI355X_GEMV=1) beside the route the same call took before
(GRB_MI355X_GEMV=0: the SpMV kernels, which read the matrix as an ordinary CSR, build a plan per matrix and, for vxm, a transposed copy), one process, operands
in HBM only.

  --what sweep   A full, FP32 PLUS_TIMES, outer x inner over 2^4 .. 2^20 each (--min-log / --max-log / --log-step) up to 2^26 entries, both layouts (N: A.mxv(u),
                 A outer x inner; T: u.vxm(A), A inner x outer), two regimes per point: `warm` — the same matrix again, so the old route's plan and transpose are
                 cached — and `fresh` — a new from_dense matrix inside every timed call, so the old route pays plan and transpose every time (and both routes pay
                 from_dense).  Five timed calls of each route after a warm-up; `noise_ms` is the larger spread (max - min) of the two, `gemv_over_spmv` the ratio of the
                 medians, `slower_beyond_noise` whether the new route lost by more than the noise, `by_default` whether the default rule admits the point.
  --what big     2^20 x 64, 64 x 2^20, 2^13 x 2^13 and 16 x 2^22 (outer x inner), FP32 / FP64 / INT8, PLUS_TIMES and MIN_PLUS, both layouts, warm: the route beside
                 a device copy of the algorithmic bytes ((m k + k + m) size: `copy_ms` moves that many, half read and half written; `over_copy` the route's time
                 over it), the yardstick, and the same product with 50 % of u absent (`holes_ms`).
Whole-call HIP-event times.  Every step runs under --step-seconds (SIGALRM) and the probe stops at the first failure.  One JSON line per measurement is appended to
--out (default profiles/gemv_full_probe.jsonl).  Run each --what as its own command under `timeout`."""
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
            sys.exit(f"gemv_probe.py: step '{self.what}' passed its limit of {self.seconds} s")
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
    """The call under GRB_MI355X_GEMV = hook.  "1": the new route.  "0": whatever the call did before the route existed; the plan is recorded either way."""
    os.environ["GRB_MI355X_GEMV"] = hook
    try:
        t, plan = runs(gb, call, reps)
    finally:
        del os.environ["GRB_MI355X_GEMV"]
    assert plan.startswith("gemv_full<") == (hook == "1"), (hook, plan)
    return t, plan


MIN_INNER = 1 << 16          # GEMV_DEFAULT_MIN_INNER of grb_gemv_geom.hpp: the default rule's row length (GrBX_gemv_geometry does not report it)
TORCH = {"FP32": "float32", "FP64": "float64", "INT8": "int8"}


def dense_tensor(rows, cols, typ):
    import torch
    dt = getattr(torch, TORCH[typ])
    if typ == "INT8":
        return torch.randint(-50, 51, (rows, cols), dtype=dt, device="cuda")
    return torch.rand((rows, cols), dtype=dt, device="cuda")


def operand(gb, T, n, holes=False, seed=0):
    rng = np.random.default_rng(seed)
    val = rng.integers(-50, 51, n).astype(T._np) if T.__name__ == "INT8" else rng.random(n).astype(T._np)
    return gb.Vector.from_dense_array(val, T, present=(rng.random(n) < 0.5).astype(np.uint8) if holes else None)


def geometry(gb):
    out = (C.c_uint64 * 10)()
    assert gb.lib.GrBX_gemv_geometry(out) == 0
    return tuple(int(v) for v in out)


def product(gb, layout, A, u, sr):
    return A.mxv(u, semiring=sr) if layout == "N" else u.vxm(A, semiring=sr)


def sweep(args):
    import pygraphblas_amd as gb
    T = gb.FP32
    min_work = geometry(gb)[7]
    logs = range(args.min_log, args.max_log + 1, args.log_step)
    for lo in logs:
        for li in logs:
            if lo + li > 26:
                continue
            m, k = 1 << lo, 1 << li
            for layout in ("N", "T"):
                rows, cols = (m, k) if layout == "N" else (k, m)
                with step(args.step_seconds, f"operands {m} {k} {layout}"):
                    X = dense_tensor(rows, cols, "FP32"); A = gb.Matrix.from_dense(X); u = operand(gb, T, k)
                for regime in ("warm", "fresh"):
                    call = (lambda: product(gb, layout, A, u, T.PLUS_TIMES)) if regime == "warm" else (lambda: product(gb, layout, gb.Matrix.from_dense(X), u, T.PLUS_TIMES))
                    rec = {"probe": "sweep", "m": m, "k": k, "layout": layout, "regime": regime, "type": "FP32", "semiring": "PLUS_TIMES", "work": m * k, "by_default": layout == "N" and k >= MIN_INNER and m * k >= min_work}
                    with step(args.step_seconds, "gemv"):
                        g, plan = routed(gb, "1", call, args.reps)
                    with step(args.step_seconds, "spmv"):
                        s, splan = routed(gb, "0", call, args.reps)
                    rec.update(gemv_runs_ms=g, gemv_ms=float(np.median(g)), gemv_plan=plan, spmv_runs_ms=s, spmv_ms=float(np.median(s)), spmv_plan=splan[:120],
                               noise_ms=round(max(max(g) - min(g), max(s) - min(s)), 4))
                    rec["gemv_over_spmv"] = round(rec["gemv_ms"] / rec["spmv_ms"], 4)
                    rec["slower_beyond_noise"] = rec["gemv_ms"] - rec["spmv_ms"] > rec["noise_ms"]
                    emit(args.out, rec)
                del A, X, u


def copy_ms(nbytes, reps):
    """Median time of a device copy that moves `nbytes` in all (half read, half written)."""
    import torch
    src = torch.empty(max(nbytes // 2, 1), dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
    times = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); a.record(); dst.copy_(src); b.record(); torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times[1:]))


def big(args):
    import torch
    import pygraphblas_amd as gb
    shapes = ((1 << 20, 64), (64, 1 << 20), (1 << 13, 1 << 13), (16, 1 << 22))
    for m, k in shapes:
        for T in (gb.FP32, gb.FP64, gb.INT8):
            if args.types and T.__name__ not in args.types:
                continue
            ts = np.dtype(T._np).itemsize
            nbytes = (m * k + k + m) * ts
            with step(args.step_seconds, "copy"):
                c = copy_ms(nbytes, args.reps)
            for layout in ("N", "T"):
                rows, cols = (m, k) if layout == "N" else (k, m)
                with step(args.step_seconds, f"operands {m} {k} {layout}"):
                    A = gb.Matrix.from_dense(dense_tensor(rows, cols, T.__name__)); u = operand(gb, T, k); uh = operand(gb, T, k, holes=True)
                for sr in ("PLUS_TIMES", "MIN_PLUS"):
                    S = getattr(T, sr)
                    rec = {"probe": "big", "m": m, "k": k, "layout": layout, "type": T.__name__, "semiring": sr, "algorithmic_bytes": nbytes, "copy_ms": round(c, 4)}
                    with step(args.step_seconds, "gemv"):
                        g, plan = routed(gb, "1", lambda: product(gb, layout, A, u, S), args.reps)
                    with step(args.step_seconds, "gemv holes"):
                        h, hplan = routed(gb, "1", lambda: product(gb, layout, A, uh, S), args.reps)
                    with step(args.step_seconds, "spmv"):
                        s, splan = routed(gb, "0", lambda: product(gb, layout, A, u, S), args.reps)
                    gm = float(np.median(g))
                    rec.update(gemv_runs_ms=g, gemv_ms=gm, gemv_plan=plan, holes_runs_ms=h, holes_ms=float(np.median(h)), holes_plan=hplan, spmv_runs_ms=s,
                               spmv_ms=float(np.median(s)), spmv_plan=splan[:120], over_copy=round(gm / c, 3), algorithmic_gb_per_s=round(nbytes / gm / 1e6, 1),
                               gemv_over_spmv=round(gm / float(np.median(s)), 4), noise_ms=round(max(max(g) - min(g), max(s) - min(s)), 4))
                    emit(args.out, rec)
                del A, u, uh
                torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["sweep", "big"], required=True)
    ap.add_argument("--min-log", type=int, default=4)
    ap.add_argument("--max-log", type=int, default=20)
    ap.add_argument("--log-step", type=int, default=2)
    ap.add_argument("--types", nargs="*", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-seconds", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gemv_full_probe.jsonl"))
    args = ap.parse_args()
    {"sweep": sweep, "big": big}[args.what](args)
