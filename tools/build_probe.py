#!/usr/bin/env python3
"""Measurement harness: build from tuples, device route (grb_build.hip) against the host route of grb_build_ops.cpp (GRB_MI355X_BUILD=0: the stable sort of an
index permutation on one thread that every call took before the device route existed), same binary, same tuples.

  --what sweep   BUILD_DEVICE_MIN_TUPLES: Matrix.from_arrays of 1e2 .. 1e7 FP64 tuples with ~5 % duplicates and dup = PLUS, from host arrays, one call on each
                 route, upload of the tuples included, the median of --reps calls after a warm-up (one call beyond 1e6 tuples on the host route).  The
                 threshold is the smallest swept size from which the device route wins at every larger size.
  --what big     R-MAT edge lists (--scales, default 20 22) with their natural duplicates, FP64 PLUS and INT64 SECOND: the device route from host arrays,
                 the device route from the tensors of rmat.edges_torch (Matrix.from_tensors: the tuples never leave HBM), and ONE call on the host route.
One JSON line per measurement is appended to --out (default profiles/build_probe.jsonl).  Run each --what as its own command under `timeout`."""
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


def timed(gb, route, reps, call, arrays=()):
    """Median wall time (ms) of `call(*arrays)` on a route, after one warm-up call; reps == 0: the single call is the measurement.  Every call gets FRESH COPIES
    of the host arrays, made outside the timed region: an ingest reads pages the runtime has not seen (and perhaps kept pinned) in an earlier repetition."""
    os.environ["GRB_MI355X_BUILD"] = route
    walls = []
    try:
        for rep in range(reps + 1):
            fresh = [a.copy() for a in arrays]
            gb.lib.GrBX_device_synchronize()
            t0 = time.perf_counter()
            result = call(*fresh)
            gb.lib.GrBX_device_synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
            assert gb.last_kernel_plan().startswith("build<") == (route == "1"), gb.last_kernel_plan()
            nvals = result.nvals
            del result
    finally:
        os.environ.pop("GRB_MI355X_BUILD", None)
    return round(float(np.median(walls[1:] if reps else walls)), 4), nvals


def sweep(args):
    import pygraphblas_amd as gb
    for n in (100, 1000, 10000, 100000, 1000000, 10000000):
        rng = np.random.default_rng(7 + n)
        dim = int(np.sqrt(4 * n)) + 1
        flat = rng.integers(0, dim * dim, n).astype(np.uint64)
        k = n // 20
        flat[rng.choice(n, k, replace=False)] = flat[rng.integers(0, n, k)]
        I, J, X = flat // np.uint64(dim), flat % np.uint64(dim), rng.random(n)
        call = lambda i, j, x: gb.Matrix.from_arrays(i, j, x, dim, dim, gb.FP64, dup=gb.FP64.PLUS)
        rec = {"probe": "sweep", "type": "FP64", "dup": "PLUS", "tuples": n, "dim": dim, "reps": args.reps, "fresh_arrays_per_call": True}
        rec["device_wall_ms_with_upload"], rec["nvals"] = timed(gb, "1", args.reps, call, (I, J, X))
        rec["host_wall_ms"], _ = timed(gb, "0", args.reps if n <= 1000000 else 0, call, (I, J, X))
        rec["device_wins"] = rec["device_wall_ms_with_upload"] < rec["host_wall_ms"]
        emit(args.out, rec)


def big(args):
    import torch
    import pygraphblas_amd as gb
    from pygraphblas_amd import rmat
    for scale in args.scales:
        n = 1 << scale
        src, dst = rmat.edges_torch(scale, "cuda")
        si, di = src.cpu().numpy().astype(np.uint64), dst.cpu().numpy().astype(np.uint64)
        for typ, op, tdt in ((gb.FP64, "PLUS", torch.float64), (gb.INT64, "SECOND", torch.int64)):
            V = torch.arange(src.numel(), device="cuda").to(tdt) % 7 + 1
            Vh = V.cpu().numpy()
            rec = {"probe": "big", "rmat_scale": scale, "tuples": int(src.numel()), "type": typ.__name__, "dup": op, "reps": args.reps, "fresh_arrays_per_call": True}
            from_host = lambda i, j, x: gb.Matrix.from_arrays(i, j, x, n, n, typ, dup=getattr(typ, op))
            rec["device_from_host_arrays_ms"], rec["nvals"] = timed(gb, "1", args.reps, from_host, (si, di, Vh))
            rec["device_from_tensors_ms"], _ = timed(gb, "1", args.reps, lambda: gb.Matrix.from_tensors(src, dst, V, n, n, typ, dup=getattr(typ, op)))
            if not args.no_host:
                rec["host_wall_ms_single_run"], _ = timed(gb, "0", 0, from_host, (si, di, Vh))
            emit(args.out, rec)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--what", choices=("sweep", "big"), required=True)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scales", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--no-host", action="store_true", help="big: skip the single host-route call")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "build_probe.jsonl"))
    args = ap.parse_args()
    {"sweep": sweep, "big": big}[args.what](args)


if __name__ == "__main__":
    main()
