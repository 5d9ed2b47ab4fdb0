#!/usr/bin/env python3
"""Measurement harness: a comparison semiring (grb_cmpsr.hip) against the one-call equivalent on the operator table, same library, same operands.

  mxv     `A.mxv(u, T.LOR_EQ, out=w)`, `T.LAND_GE` and `T.ANY_EQ` through k_cmpsr_rows against `T.MAX_ISEQ`, `T.MIN_ISGE` and `T.ANY_ISEQ` through the table
          route (the SpMV kernels), all into a BOOL vector w of the matrix's size: the table route writes its n-vector in T and casts it on the way out.
          `T.LXOR_EQ` has no one-call equivalent on the table: its time is recorded alone.
The operands are labels: R-MAT of --scales (default 20 and 22), 16 edges per vertex, the matrix's values and a full u drawn from 0..7 in --types (default INT64
and FP32), resident in HBM.  Every figure is the HIP-event time of a whole call; the two versions of a pair run alternately, --reps times each (default 5) after a
warm-up round, and the record carries the median, the minimum and the maximum of each, so the run-to-run spread stands beside the difference.  The table route's
kernels are the ones the library had before the comparison semirings existed (the plan string of each call is recorded).  One JSON line per measurement is
appended to --out (default profiles/cmpsr_probe.jsonl).  No ratio is required of either."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
from possr_probe import alternate, stats
from userop_probe import emit

PAIRS = [("LOR_EQ", "MAX_ISEQ", True), ("LAND_GE", "MIN_ISGE", True), ("ANY_EQ", "ANY_ISEQ", False)]      # (comparison semiring, table semiring, values must be equal)


def labelled_rmat(gb, scale, seed, T):
    from pygraphblas_amd import rmat as R
    rp, ci = R.csr_numpy(scale, seed=seed)
    x = np.random.default_rng(seed).integers(0, 8, len(ci)).astype(T._np)
    return gb.Matrix.from_csr(T, 1 << scale, 1 << scale, rp, ci, x)          # HBM only


def run(args, scale, tname):
    import pygraphblas_amd as gb
    lib, T = gb.lib, getattr(gb, tname)
    A = labelled_rmat(gb, scale, 42, T)
    n = 1 << scale
    u = gb.Vector.from_arrays(np.arange(n, dtype=np.uint64), np.random.default_rng(7).integers(0, 8, n).astype(T._np), n, T)
    base = {"scale": scale, "type": tname, "entries_A": int(A.nvals), "reps": args.reps, "probe": "mxv", "output": "BOOL vector"}
    for cmp_name, table_name, same_values in PAIRS:
        new_sr, old_sr = getattr(T, cmp_name), getattr(T, table_name)
        plans = {}

        def call(sr, key):
            w = A.mxv(u, sr, out=gb.Vector.sparse(gb.BOOL, n))
            plans[key] = gb.last_kernel_plan()
            return w
        times, last = alternate(lib, {"cmpsr": lambda: call(new_sr, "cmpsr"), "table": lambda: call(old_sr, "table")}, args.reps)
        (gi, gx), (wi, wx) = last["cmpsr"].to_arrays(), last["table"].to_arrays()
        same = bool(np.array_equal(gi, wi) and (not same_values or np.array_equal(gx, wx)))
        emit(args.out, dict(base, operation=f"A.mxv(u, {cmp_name}) against A.mxv(u, {table_name})", entries_out=int(last["cmpsr"].nvals),
                            equal_results=same, values_compared=same_values, cmpsr=stats(times["cmpsr"]), table=stats(times["table"]),
                            cmpsr_over_table=round(float(np.median(times["cmpsr"]) / np.median(times["table"])), 3), plan=plans["cmpsr"][:160],
                            table_plan=plans["table"][:160]))
    plans = {}
    times, last = alternate(lib, {"cmpsr": lambda: A.mxv(u, T.LXOR_EQ, out=gb.Vector.sparse(gb.BOOL, n))}, args.reps)
    emit(args.out, dict(base, operation="A.mxv(u, LXOR_EQ): no one-call equivalent on the table", entries_out=int(last["cmpsr"].nvals),
                        true_entries=int(last["cmpsr"].to_arrays()[1].sum()), cmpsr=stats(times["cmpsr"]), plan=gb.last_kernel_plan()[:160]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--types", nargs="+", default=["INT64", "FP32"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cmpsr_probe.jsonl"))
    args = ap.parse_args()
    import pygraphblas_amd as gb
    if not gb.device_info()["ok"]:
        sys.exit("cmpsr_probe.py measures on the GPU: no HIP device")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for s in args.scales:
        for t in args.types:
            run(args, s, t)
