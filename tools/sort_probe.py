#!/usr/bin/env python3
"""Measurement harness: sort and top-k on the device (grb_sort.hip), the binned route against the segmented-radix-sort route of the same call
(GRB_MI355X_SORT=prim), the host route (GRB_MI355X_SORT=0, --host: one call) and a device-to-device copy of the bytes the call has to move.

  --what rows    GxB_Matrix_sort (C and P) of an R-MAT matrix (--scale, --type FP64 | INT32) that lives in HBM only
  --what topk    GrBX_Matrix_select_topk with k = 8 of the same matrix
  --what vector  GxB_Vector_sort (w and p) of 2^--scale FP32 entries (default 26), every position present
Each call is timed between two device synchronisations (HIP events on the library stream); the median of --reps calls after a warm-up.  The copy floor moves
keys + positions + outputs: per entry (key bytes + 4) + (4 + value bytes) + (4 + 8) for a sort, (key bytes + 4) + 1 + (4 + value bytes) for a top-k.
One JSON line per measurement is appended to --out (default profiles/sort_probe.jsonl).  Run each invocation as its own command under `timeout`."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def emit(out, rec):
    print(json.dumps(rec), flush=True)
    with open(out, "a") as f:
        f.write(json.dumps(rec) + "\n")


def timed(gb, call, reps):
    """Median event time of `reps` calls after one warm-up, and the plan string of the last."""
    times = []
    for _ in range(reps + 1):
        gb.lib.GrBX_device_synchronize()
        gb.lib.GrBX_timer_start()
        out = call()
        ms = C.c_float(0)
        gb.lib.GrBX_timer_stop(C.byref(ms))
        plan = gb.last_kernel_plan()
        del out
        times.append(ms.value)
    return round(float(np.median(times[1:])), 4), plan


def copy_floor_ms(nbytes, reps):
    import torch
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    times = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    del src, dst
    return round(float(np.median(times[1:])), 4)


def routes(gb, rec, call, reps, host):
    for label, env in (("binned", None), ("prim", "prim")) + ((("host", "0"),) if host else ()):
        if env is None:
            os.environ.pop("GRB_MI355X_SORT", None)
        else:
            os.environ["GRB_MI355X_SORT"] = env
        ms, plan = timed_once(gb, call) if label == "host" else timed(gb, call, reps)
        rec[label + "_ms"] = ms
        if label != "host":
            rec[label + "_plan"] = plan
    os.environ.pop("GRB_MI355X_SORT", None)
    rec["binned_over_prim"] = round(rec["binned_ms"] / rec["prim_ms"], 4)
    rec["binned_over_copy"] = round(rec["binned_ms"] / rec["copy_floor_ms"], 2)


def timed_once(gb, call):
    gb.lib.GrBX_device_synchronize()
    gb.lib.GrBX_timer_start()
    out = call()
    ms = C.c_float(0)
    gb.lib.GrBX_timer_stop(C.byref(ms))
    del out
    return round(ms.value, 4), ""


def matrix(args, gb):
    from pygraphblas_amd import rmat
    typ = getattr(gb, args.type)
    n = 1 << args.scale
    rp, col = rmat.csr_numpy(args.scale, seed=42)
    rng = np.random.default_rng(args.scale)
    vals = rng.standard_normal(len(col)).astype(typ._np) if args.type.startswith("FP") else rng.integers(-(1 << 30), 1 << 30, len(col)).astype(typ._np)
    A = gb.Matrix.from_csr(typ, n, n, rp.astype(np.uint32), col.astype(np.uint32), vals)      # HBM only
    return A, typ, n, int(len(col)), np.diff(rp.astype(np.int64))


def rows(args):
    import pygraphblas_amd as gb
    A, typ, n, nnz, lens = matrix(args, gb)
    ts = typ._np().itemsize
    kb = 8 if ts == 8 else 4
    topk = args.what == "topk"
    nbytes = nnz * ((kb + 4) + 1 + (4 + ts)) if topk else nnz * ((kb + 4) + (4 + ts) + (4 + 8))
    rec = {"probe": args.what, "scale": args.scale, "type": args.type, "rows": n, "entries": nnz, "rows_le_64": int((lens <= 64).sum()), "longest_row": int(lens.max()),
           "copy_bytes": nbytes, "copy_floor_ms": copy_floor_ms(nbytes, args.reps)}
    call = (lambda: A.topk(8)) if topk else (lambda: A.sort())
    routes(gb, rec, call, args.reps, args.host)
    for edges in args.edges or ():                                   # the same call with other bin edges (GRB_MI355X_SORT_EDGES): which bin wins from where
        os.environ["GRB_MI355X_SORT_EDGES"] = edges
        ms, plan = timed(gb, call, args.reps)
        rec["edges_" + edges + "_ms"] = ms
        rec["edges_" + edges + "_bins"] = plan[plan.index("wave="):plan.index(">")]
    os.environ.pop("GRB_MI355X_SORT_EDGES", None)
    emit(args.out, rec)


def vector(args):
    import pygraphblas_amd as gb
    n = 1 << args.scale
    x = np.random.default_rng(1).standard_normal(n).astype(np.float32)
    u = gb.Vector.from_dense_array(x, gb.FP32)
    nbytes = n * ((4 + 4) + (4 + 1) + (8 + 1))
    rec = {"probe": "vector", "entries": n, "type": "FP32", "copy_bytes": nbytes, "copy_floor_ms": copy_floor_ms(nbytes, args.reps)}
    ms, plan = timed(gb, lambda: u.sort(), args.reps)
    rec.update(device_ms=ms, plan=plan, device_over_copy=round(ms / rec["copy_floor_ms"], 2))
    if args.host:
        os.environ["GRB_MI355X_SORT"] = "0"
        rec["host_ms"] = timed_once(gb, lambda: u.sort())[0]
        os.environ.pop("GRB_MI355X_SORT", None)
    emit(args.out, rec)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="rows", choices=["rows", "topk", "vector"])
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--type", default="FP64", choices=["FP64", "INT32"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--edges", nargs="*", help='bin edges "W,L" to time besides the chosen ones, e.g. 64,64 0,4096 64,512')
    ap.add_argument("--host", action="store_true", help="also one call on the host route (slow: a map insertion per entry)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sort_probe.jsonl"))
    args = ap.parse_args()
    import pygraphblas_amd as gb
    if not gb.device_info()["ok"]:
        sys.exit("sort_probe.py measures on the GPU: no HIP device")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    {"rows": rows, "topk": rows, "vector": vector}[args.what](args)
