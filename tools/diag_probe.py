#!/usr/bin/env python3
"""Measurement harness: diagonals, device route (grb_diag.hip) against the host route of grb_diag_ops.cpp (GRB_MI355X_DIAG=0: what every call took before the
device route existed), same binary, fresh inputs per call.

  --what sweep   the thresholds of the dispatch of GxB_Matrix_diag (Matrix.from_diag) and GxB_Vector_diag (Matrix.vector_diag): operands of 1e2 .. 1e6 FP32
                 entries whose only valid image is the HOST mirror — a vector with every second position present; a matrix with that diagonal and two
                 more entries per row — one call on each route, upload included, the median of --reps calls after a warm-up.  The threshold of an entry
                 point is the smallest decade from which the device route wins and keeps winning.
  --what big     operands that live in HBM only: `A.vector_diag()` and `Matrix.from_diag(A.reduce_vector())` of R-MAT matrices (--scales, default 20 22;
                 self-loops added so that the diagonal is not empty), whole-call HIP-event time, the mean of --reps calls after a warm-up.
One JSON line per measurement is appended to --out (default profiles/diag_probe.jsonl).  Run each --what as its own command under `timeout`."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def emit(out, rec):
    print(json.dumps(rec), flush=True)
    with open(out, "a") as f:
        f.write(json.dumps(rec) + "\n")


def timed_routes(gb, rec, reps, make, call, plan_prefix):
    for route in ("1", "0"):
        os.environ["GRB_MI355X_DIAG"] = route
        walls = []
        for rep in range(reps + 1):                                 # the first repetition is the warm-up
            operand = make()                                        # host mirror only: the device route uploads inside the call
            gb.lib.GrBX_device_synchronize()
            t0 = time.perf_counter()
            result = call(operand)
            gb.lib.GrBX_device_synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
            assert gb.last_kernel_plan().startswith(plan_prefix) == (route == "1"), gb.last_kernel_plan()
            del operand, result
        rec["device_wall_ms_with_upload" if route == "1" else "host_wall_ms"] = round(float(np.median(walls[1:])), 4)
    rec["device_wins"] = rec["device_wall_ms_with_upload"] < rec["host_wall_ms"]
    os.environ.pop("GRB_MI355X_DIAG", None)


def sweep(args):
    import pygraphblas_amd as gb
    for entries in (100, 1000, 10000, 100000, 1000000):
        rng = np.random.default_rng(3 + entries)
        n = 2 * entries
        idx = np.arange(0, n, 2, dtype=np.uint64)
        x = rng.random(entries).astype(np.float32)
        rec = {"probe": "sweep", "entry_point": "GxB_Matrix_diag", "operand_entries": entries, "n": n}
        timed_routes(gb, rec, args.reps, lambda: gb.Vector.from_arrays(idx, x, n, gb.FP32), lambda v: gb.Matrix.from_diag(v), "diag_matrix<")
        emit(args.out, rec)
        rows = entries // 3 + 1                                     # three entries per row: the diagonal of every second row, two others
        r = np.arange(rows, dtype=np.uint64)
        I = np.repeat(r, 3)
        J = np.stack([np.where(r % 2 == 0, r, (r + 1) % rows), (r + 2) % rows, (r + 5) % rows], axis=1)
        J.sort(axis=1)
        keep = np.concatenate([[True], (I[1:] != I[:-1]) | (J.ravel()[1:] != J.ravel()[:-1])])
        I, J = I[keep], J.ravel()[keep]
        X = rng.random(len(I)).astype(np.float32)
        rec = {"probe": "sweep", "entry_point": "GxB_Vector_diag", "operand_entries": int(len(I)), "n": int(rows)}
        timed_routes(gb, rec, args.reps, lambda: gb.Matrix.from_arrays(I, J, X, rows, rows, gb.FP32), lambda A: A.vector_diag(), "diag_vector<")
        emit(args.out, rec)


def big(args):
    import pygraphblas_amd as gb
    from pygraphblas_amd import rmat
    lib = gb.lib
    os.environ.pop("GRB_MI355X_DIAG", None)                         # default routing: HBM-only operands take the device route by themselves
    for scale in args.scales:
        n = 1 << scale
        rp, col = rmat.csr_numpy(scale, seed=42)
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp.astype(np.int64)))
        keys = np.unique(np.concatenate([rows * n + col.astype(np.int64), np.arange(0, n, 2, dtype=np.int64) * (n + 1)]))      # + a self-loop on every second vertex
        rows, col = np.divmod(keys, n)
        rp = np.zeros(n + 1, np.int64); np.add.at(rp, rows + 1, 1)
        A = gb.Matrix.from_csr(gb.FP32, n, n, np.cumsum(rp).astype(np.uint32), col.astype(np.uint32), np.ones(len(col), np.float32))      # HBM only
        d = A.reduce_vector()                                       # the out-degrees: in HBM only
        for name, call, prefix in (("A.vector_diag()", lambda: A.vector_diag(), "diag_vector<"), ("Matrix.from_diag(A.reduce_vector())", lambda: gb.Matrix.from_diag(d), "diag_matrix<")):
            times = []
            for rep in range(args.reps + 1):                        # the first repetition is the warm-up (code object, pool)
                lib.GrBX_device_synchronize()
                lib.GrBX_timer_start()
                out = call()
                ms = C.c_float(0); lib.GrBX_timer_stop(C.byref(ms))
                plan = gb.last_kernel_plan()
                nvals = int(out.nvals)
                del out
                times.append(ms.value)
            assert plan.startswith(prefix), plan
            emit(args.out, {"probe": "big", "call": name, "scale": scale, "matrix_entries": int(len(col)), "result_entries": nvals,
                            "whole_call_event_ms": round(float(np.mean(times[1:])), 4), "plan": plan})
        del A, d


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="sweep")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scales", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_probe.jsonl"))
    args = ap.parse_args()
    import pygraphblas_amd as gb
    if not gb.device_info()["ok"]:
        sys.exit("diag_probe.py measures on the GPU: no HIP device")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    {"sweep": sweep, "big": big}[args.what](args)
