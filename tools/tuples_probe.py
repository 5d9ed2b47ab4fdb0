#!/usr/bin/env python3
"""Measurement harness: extractTuples in HBM (grb_tuples.hip; Matrix.to_tensors / Vector.to_tensors) of containers that live in HBM only, against
  (a) to_arrays() of a dup(): today's route to the host — the download, the host mirror, the per-entry copy (the dup itself is made outside the timed region), and
  (b) a device-to-device copy that moves as many bytes as the kernels read plus write (a copy of B bytes reads B and writes B, so B = half that traffic): the floor.

  --what big     R-MAT-20 / 22 (--scales) FP64 and BOOL matrices, and a vector of 2^26 positions (--vector-log2) at 1 %, 50 % and 100 % density.
  --what sweep   FP64 matrices of 1e3 .. 1e7 entries.
Every figure is the median of --reps calls after a warm-up, wall clock with a device synchronisation on both sides.  One JSON line per measurement is appended to
--out (default profiles/tuples_probe.jsonl).  Run each --what as its own command under `timeout`."""
import argparse
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


def timed(gb, reps, call, before=None):
    """Median wall time (ms) of call(before()) after one warm-up; `before` runs outside the timed region."""
    import torch
    walls = []
    for _ in range(reps + 1):
        arg = before() if before else None
        torch.cuda.synchronize(); gb.lib.GrBX_device_synchronize()
        t0 = time.perf_counter()
        r = call(arg) if before else call()
        torch.cuda.synchronize(); gb.lib.GrBX_device_synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
        del r, arg
    return round(float(np.median(walls[1:])), 4)


def copy_floor_ms(gb, reps, traffic_bytes):
    import torch
    half = max(int(traffic_bytes) // 2, 16)
    src = torch.zeros(half, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
    return timed(gb, reps, lambda: dst.copy_(src))


def matrix_record(gb, args, A, ts, extra):
    nv = A.nvals
    rec = dict(extra, nvals=nv, value_bytes=ts, reps=args.reps)
    rec["to_tensors_ms"] = timed(gb, args.reps, A.to_tensors)
    assert gb.last_kernel_plan() == "tuples<on=matrix,i=1,j=1,x=1> k_tuples_csr", gb.last_kernel_plan()
    rec["to_tensors_indices_only_ms"] = timed(gb, args.reps, lambda: A.to_tensors(values=False))
    traffic = nv * (4 + ts) + nv * (16 + ts) + (A.nrows + 1) * 4      # col + val read, I + J + X written, the row pointer once
    rec["traffic_bytes"] = traffic
    rec["copy_floor_ms"] = copy_floor_ms(gb, args.reps, traffic)
    rec["ratio_to_copy_floor"] = round(rec["to_tensors_ms"] / rec["copy_floor_ms"], 3)
    if not args.no_host:
        rec["host_route_to_arrays_of_dup_ms"] = timed(gb, min(args.reps, 1) if nv > 3e7 else args.reps, lambda d: d.to_arrays(), A.dup)
    emit(args.out, rec)


def rmat_matrix(gb, scale, typ, tdt):
    import torch
    from pygraphblas_amd import rmat
    rowptr, cols = rmat.csr_torch(scale, "cuda")
    vals = (torch.arange(cols.numel(), device="cuda") % 7 + 1).to(tdt)
    torch.cuda.synchronize()
    n = 1 << scale
    return gb.Matrix.from_csr(typ, n, n, rowptr.data_ptr(), cols.data_ptr(), (vals.data_ptr(), int(cols.numel())), device=True)


def big(args):
    import torch
    import pygraphblas_amd as gb
    for scale in args.scales:
        for typ, tdt, ts in ((gb.FP64, torch.float64, 8), (gb.BOOL, torch.bool, 1)):
            A = rmat_matrix(gb, scale, typ, tdt)
            matrix_record(gb, args, A, ts, {"probe": "big", "on": "matrix", "rmat_scale": scale, "type": typ.__name__})
            del A
    n = 1 << args.vector_log2
    for density in (0.01, 0.5, 1.0):
        val = torch.rand(n, dtype=torch.float64, device="cuda")
        pres = (torch.rand(n, device="cuda") < density).to(torch.uint8) if density < 1.0 else None
        torch.cuda.synchronize()
        v = gb.Vector.from_dense_array((val.data_ptr(), n), gb.FP64, present=pres.data_ptr() if pres is not None else None, device=True)
        nv = v.nvals
        rec = {"probe": "big", "on": "vector", "positions": n, "density": density, "type": "FP64", "nvals": nv, "reps": args.reps}
        rec["to_tensors_ms"] = timed(gb, args.reps, v.to_tensors)
        rec["plan"] = gb.last_kernel_plan()
        traffic = (0 if density == 1.0 else 2 * n) + nv * 8 + nv * 16      # the presence bytes twice (count, scatter), the present values read, I + X written
        rec["traffic_bytes"] = traffic
        rec["copy_floor_ms"] = copy_floor_ms(gb, args.reps, traffic)
        rec["ratio_to_copy_floor"] = round(rec["to_tensors_ms"] / rec["copy_floor_ms"], 3)
        if not args.no_host:
            rec["host_route_to_arrays_of_dup_ms"] = timed(gb, min(args.reps, 1), lambda d: d.to_arrays(), v.dup)
        emit(args.out, rec)
        del v, val, pres


def sweep(args):
    import pygraphblas_amd as gb
    for n in (1000, 10000, 100000, 1000000, 10000000):
        rng = np.random.default_rng(7 + n)
        dim = int(np.sqrt(4 * n)) + 1
        flat = np.unique(rng.integers(0, dim * dim, n))
        rowptr = np.zeros(dim + 1, np.int64); np.add.at(rowptr, flat // dim + 1, 1)
        A = gb.Matrix.from_csr(gb.FP64, dim, dim, np.cumsum(rowptr).astype(np.uint32), (flat % dim).astype(np.uint32), rng.random(len(flat)))
        matrix_record(gb, args, A, 8, {"probe": "sweep", "on": "matrix", "type": "FP64", "dim": dim})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--what", choices=("sweep", "big"), required=True)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scales", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--vector-log2", type=int, default=26)
    ap.add_argument("--no-host", action="store_true", help="skip the host route (to_arrays of a dup)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tuples_probe.jsonl"))
    args = ap.parse_args()
    {"sweep": sweep, "big": big}[args.what](args)


if __name__ == "__main__":
    main()
