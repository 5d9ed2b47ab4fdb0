#!/usr/bin/env python3
"""Measurement harness: GrB_mxm of two FULL operands — the gemm_full route (GRB_MI355X_GEMM=1) beside the route the same call took before (GRB_MI355X_GEMM=0:
spmm_full, which reads the left operand as an ordinary CSR, from 2^18 products; the hash product below that), one process, operands in HBM only.

  --what sweep   X full m x k, W full k x n, FP32 PLUS_TIMES, m = 2^10 .. 2^20 (--min-log-m / --max-log-m / --log-m-step), k in 16, 64, 256, n in 2, 16, 64, 256,
                 where m n < 2^32 and the operands and two results fit --max-bytes.  Five timed calls of each route after a warm-up; `noise_ms` is the larger spread
                 (max - min) of the two, `gemm_over_spmm` the ratio of the medians, `slower_beyond_noise` whether the new route lost by more than the noise,
                 `by_default` whether the default rule admits the point (GrBX_gemm_geometry's threshold and GEMM_MIN_TILES tiles of the result).  The yardstick is not run beyond --max-yardstick-work
                 multiply-adds.
  --what big     m = 2^20, k = n = 64 and m = 2^22, k = 64, n = 16, FP32 and FP64, PLUS_TIMES and MIN_PLUS: the route beside a device copy of the algorithmic bytes
                 ((m k + k n + m n) size + 4 m n: `copy_ms` moves that many, half read and half written; `over_copy` the route's time over it), `peak_share` the
                 2 m n k operations per second over the FP32 vector peak of 157.3e12, the yardstick, and the NT layout (W handed over as n x k with desc T1) beside NN.
Whole-call HIP-event times.  Every step runs under --step-seconds (SIGALRM) and the probe stops at the first failure.  One JSON line per measurement is appended to
--out (default profiles/gemm_full_probe.jsonl).  Run each --what as its own command under `timeout`."""
import argparse
import ctypes as C
import json
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

FP32_VECTOR_PEAK = 157.3e12
MIN_TILES = 16              # GEMM_MIN_TILES of grb_gemm_geom.hpp: the default rule's tile count (GrBX_gemm_geometry does not report it)


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
            sys.exit(f"gemm_probe.py: step '{self.what}' passed its limit of {self.seconds} s")
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


def routed(gb, hook, call, reps, spmm_by_default=True):
    """The call under GRB_MI355X_GEMM = hook.  "1": the new route.  "0": whatever the call did before the route existed — spmm_full where its own default rule
    admits the call (`spmm_by_default`), the hash product below it; the plan is recorded either way."""
    os.environ["GRB_MI355X_GEMM"] = hook
    try:
        t, plan = runs(gb, call, reps)
    finally:
        del os.environ["GRB_MI355X_GEMM"]
    if hook == "1":
        assert plan.startswith("gemm_full<"), (hook, plan)
    else:
        assert "gemm_full<" not in plan and (plan.startswith("spmm_full<") or not spmm_by_default), (hook, plan)
    return t, plan


def torch_dtype(typ):
    import torch
    return {np.float32: torch.float32, np.float64: torch.float64}[typ._np]


def full_operand(gb, rows, cols, typ):
    import torch
    return gb.Matrix.from_dense(torch.rand((rows, cols), dtype=torch_dtype(typ), device="cuda"))


def geometry(gb):
    out = (C.c_uint64 * 9)()
    assert gb.lib.GrBX_gemm_geometry(out) == 0
    return tuple(int(v) for v in out)


def sweep(args):
    import pygraphblas_amd as gb
    T = gb.FP32
    g = geometry(gb); wide, tall, min_work, talln = g[0:2], g[2:4], g[7], g[8]
    for log_m in range(args.min_log_m, args.max_log_m + 1, args.log_m_step):
        m = 1 << log_m
        for k in (16, 64, 256):
            for n in (2, 16, 64, 256):
                if m * n >= (1 << 32) - 16 or (m * k + k * n) * 8 + 2 * m * n * 8 > args.max_bytes:
                    continue
                with step(args.step_seconds, f"operands {m} {k} {n}"):
                    X = full_operand(gb, m, k, T); W = full_operand(gb, k, n, T)
                work = m * k * n
                tiles = -(-m // tall[0]) * -(-n // tall[1]) if n <= talln else -(-m // wide[0]) * -(-n // wide[1])
                spmm_rule = n >= 2 and work >= min_work                           # spmm_full's own default rule on a full left operand: nnz(A) n = m k n, the same count
                rec = {"probe": "sweep", "m": m, "k": k, "n": n, "type": "FP32", "semiring": "PLUS_TIMES", "work": work, "tiles": tiles, "by_default": spmm_rule and tiles >= MIN_TILES}
                with step(args.step_seconds, "gemm"):
                    g, plan = routed(gb, "1", lambda: X.mxm(W, semiring=T.PLUS_TIMES), args.reps)
                rec.update(gemm_runs_ms=g, gemm_ms=float(np.median(g)), gemm_plan=plan)
                if work <= args.max_yardstick_work:
                    with step(args.step_seconds, "spmm"):
                        s, splan = routed(gb, "0", lambda: X.mxm(W, semiring=T.PLUS_TIMES), args.reps, spmm_by_default=spmm_rule)
                    rec.update(spmm_runs_ms=s, spmm_ms=float(np.median(s)), spmm_plan=splan[:120], noise_ms=round(max(max(g) - min(g), max(s) - min(s)), 4))
                    rec["gemm_over_spmm"] = round(rec["gemm_ms"] / rec["spmm_ms"], 4)
                    rec["slower_beyond_noise"] = rec["gemm_ms"] - rec["spmm_ms"] > rec["noise_ms"]
                else:
                    rec["spmm_ms"] = None                                         # not run: beyond --max-yardstick-work
                emit(args.out, rec)
                del X, W


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
    from pygraphblas_amd import descriptor as D
    for log_m, k, n in ((20, 64, 64), (22, 64, 16)):
        if log_m > args.max_log_m:
            continue
        m = 1 << log_m
        for T in (gb.FP32, gb.FP64):
            with step(args.step_seconds, f"operands {m} {k} {n}"):
                X = full_operand(gb, m, k, T); W = full_operand(gb, k, n, T)
                Wt = gb.Matrix.from_dense(W.to_dense_tensor().t().contiguous())
            ts = np.dtype(T._np).itemsize
            nbytes = (m * k + k * n + m * n) * ts + 4 * m * n
            with step(args.step_seconds, "copy"):
                c = copy_ms(nbytes, args.reps)
            for sr in ("PLUS_TIMES", "MIN_PLUS"):
                rec = {"probe": "big", "m": m, "k": k, "n": n, "type": T.__name__, "semiring": sr, "work": m * k * n, "algorithmic_bytes": nbytes, "copy_ms": round(c, 4)}
                with step(args.step_seconds, "gemm NN"):
                    g, plan = routed(gb, "1", lambda: X.mxm(W, semiring=getattr(T, sr)), args.reps)
                with step(args.step_seconds, "gemm NT"):
                    t, tplan = routed(gb, "1", lambda: X.mxm(Wt, semiring=getattr(T, sr), out=gb.Matrix.sparse(T, m, n), desc=D.T1), args.reps)
                with step(args.step_seconds, "spmm"):
                    s, splan = routed(gb, "0", lambda: X.mxm(W, semiring=getattr(T, sr)), args.reps)
                gm = float(np.median(g))
                rec.update(gemm_runs_ms=g, gemm_ms=gm, gemm_plan=plan, nt_runs_ms=t, nt_ms=float(np.median(t)), nt_plan=tplan, spmm_runs_ms=s, spmm_ms=float(np.median(s)),
                           spmm_plan=splan[:120], over_copy=round(gm / c, 3), algorithmic_gb_per_s=round(nbytes / gm / 1e6, 1),
                           peak_share=round(2.0 * m * k * n / (gm * 1e-3) / FP32_VECTOR_PEAK, 4), gemm_over_spmm=round(gm / float(np.median(s)), 4),
                           noise_ms=round(max(max(g) - min(g), max(s) - min(s)), 4))
                emit(args.out, rec)
            del X, W, Wt
            torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["sweep", "big"], required=True)
    ap.add_argument("--min-log-m", type=int, default=10)
    ap.add_argument("--max-log-m", type=int, default=None)
    ap.add_argument("--log-m-step", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-bytes", type=int, default=16 << 30)
    ap.add_argument("--max-yardstick-work", type=int, default=1 << 40)
    ap.add_argument("--step-seconds", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gemm_full_probe.jsonl"))
    args = ap.parse_args()
    if args.max_log_m is None:
        args.max_log_m = 20 if args.what == "sweep" else 22
    {"sweep": sweep, "big": big}[args.what](args)
