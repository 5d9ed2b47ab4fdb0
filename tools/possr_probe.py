#!/usr/bin/env python3
"""Measurement harness: a positional semiring (grb_possr.hip) against the workaround it replaces, on the same library and the same operands.

  vxm     one `u.vxm(A, INT64.MIN_SECONDI)` over a full frontier (every position of u present) against `u.vxm(Ai, INT64.MIN_SECOND)` with
          Ai = A.apply(INT64.POSITIONI) — the copy of A with an 8-byte row index per entry, made once and NOT timed.
  bfs     the BFS-parent loop from vertex `--source`: `q<!p, structural, replace> = q (+).secondi A ; p<q, structural> = q` until q is empty, with
          MIN_SECONDI over A against MIN_SECOND over Ai (both give the smallest parent: the results must be equal), and with ANY_SECONDI over A.
R-MAT of --scales (default 20 and 22), 16 edges per vertex, an FP64 matrix that lives in HBM.  Every figure is the HIP-event time of whole calls; the versions of a
pair are run alternately, --reps times each after a warm-up pass, and the record carries the median, the minimum and the maximum of each, so the run-to-run spread
stands beside the difference.  One JSON line per measurement is appended to --out (default profiles/possr_probe.jsonl).  No ratio is required of either."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
from userop_probe import emit, rmat


def event_ms(lib, fn):
    lib.GrBX_device_synchronize()
    lib.GrBX_timer_start()
    r = fn()
    ms = C.c_float(0)
    lib.GrBX_timer_stop(C.byref(ms))
    return ms.value, r


def alternate(lib, calls, reps):
    """{name: [ms, ...]} of `reps` rounds that run every call once, in turn, after one warm-up round; and the last result of each."""
    times, last = {k: [] for k in calls}, {}
    for rnd in range(reps + 1):
        for name, fn in calls.items():
            ms, r = event_ms(lib, fn)
            if rnd:
                times[name].append(ms)
            last[name] = r
    return times, last


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(min(ms)), 4), "max_ms": round(float(max(ms)), 4)}


def bfs_parents(gb, A, sr, source):
    n, D = A.nrows, gb.descriptor
    p = gb.Vector.from_lists([source], [source], n, gb.INT64)
    q = gb.Vector.from_lists([source], [source], n, gb.INT64)
    levels = 0
    while True:
        q.vxm(A, sr, out=q, mask=p, desc=D.RSC)
        if q.nvals == 0:
            return p, levels
        p.assign(q, mask=q, desc=D.S)
        levels += 1


def run(args, scale):
    import pygraphblas_amd as gb
    lib, T = gb.lib, gb.INT64
    A = rmat(gb, scale, 42)
    n = 1 << scale
    Ai = A.apply(T.POSITIONI, out=gb.Matrix.sparse(T, n, n))                 # the workaround's copy: made once, outside every timed window
    u = gb.Vector.from_arrays(np.arange(n, dtype=np.uint64), np.ones(n, np.int64), n, T)
    base = {"scale": scale, "entries_A": int(A.nvals), "reps": args.reps}

    times, last = alternate(lib, {"possr": lambda: u.vxm(A, T.MIN_SECONDI), "workaround": lambda: u.vxm(Ai, T.MIN_SECOND)}, args.reps)
    plan = gb.last_kernel_plan()
    same = all(np.array_equal(a, b) for a, b in zip(last["possr"].to_arrays(), last["workaround"].to_arrays()))
    u.vxm(A, T.MIN_SECONDI)
    emit(args.out, dict(base, probe="vxm", operation="u.vxm(A, MIN_SECONDI), full u", entries_out=int(last["possr"].nvals), equal_results=bool(same),
                        possr=stats(times["possr"]), workaround_MIN_SECOND_over_POSITIONI=stats(times["workaround"]),
                        possr_over_workaround=round(float(np.median(times["possr"]) / np.median(times["workaround"])), 3), plan=gb.last_kernel_plan()[:160],
                        workaround_plan=plan[:160]))

    calls = {"possr_MIN": lambda: bfs_parents(gb, A, T.MIN_SECONDI, args.source)[0], "workaround_MIN": lambda: bfs_parents(gb, Ai, T.MIN_SECOND, args.source)[0],
             "possr_ANY": lambda: bfs_parents(gb, A, T.ANY_SECONDI, args.source)[0]}
    times, last = alternate(lib, calls, args.reps)
    same = all(np.array_equal(a, b) for a, b in zip(last["possr_MIN"].to_arrays(), last["workaround_MIN"].to_arrays()))
    _p, levels = bfs_parents(gb, A, T.MIN_SECONDI, args.source)
    emit(args.out, dict(base, probe="bfs", operation="BFS parents: q<!p,s,r> = q.vxm(A); p<q,s> = q", source=args.source, levels=levels, reached=int(last["possr_MIN"].nvals),
                        equal_results=bool(same), possr_MIN_SECONDI=stats(times["possr_MIN"]), workaround_MIN_SECOND_over_POSITIONI=stats(times["workaround_MIN"]),
                        possr_ANY_SECONDI=stats(times["possr_ANY"]),
                        possr_over_workaround=round(float(np.median(times["possr_MIN"]) / np.median(times["workaround_MIN"])), 3)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--source", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "possr_probe.jsonl"))
    args = ap.parse_args()
    import pygraphblas_amd as gb
    if not gb.device_info()["ok"]:
        sys.exit("possr_probe.py measures on the GPU: no HIP device")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for s in args.scales:
        run(args, s)
