#!/usr/bin/env python3
"""Measurement harness: the Kronecker product, device route (grb_kron.hip) against the host route of grb_kron_ops.cpp (GRB_MI355X_KRON=0: what every
call took before the device route existed), same binary, fresh inputs per call.

  --what sweep   the threshold of GrB_Matrix_kronecker_BinaryOp's dispatch: uniform random FP32 operands whose only valid image is the HOST mirror,
                 nnz(A) nnz(B) = 1e2 .. 1e6; one call on each route, upload included, the median of --reps calls after a warm-up.  The threshold is
                 the smallest decade at which the device route wins.
  --what big     operands that live in HBM only, products of ~6.4e7 and ~5e8 entries, FP32 and FP64: the device time of k_kron_fill alone (HIP events
                 around its launch: GRB_MI355X_KRON_TIME=1, GrBX_kron_fill_ms) as a store rate over nnz(T) (4 + sizeof T) bytes, the whole call's
                 HIP-event time, and beside them the plain store stream of the same number of bytes (a torch fill, as tools/membw_probe.py measures it).
One JSON line per measurement is appended to --out (default profiles/kron_probe.jsonl).  Run each --what as its own command under `timeout`."""
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


def random_coo(rng, n, nnz, dt):
    flat = np.sort(rng.choice(n * n, size=nnz, replace=False))
    I, J = np.divmod(flat, n)
    return I.astype(np.uint64), J.astype(np.uint64), rng.random(nnz).astype(dt)


def sweep(args):
    import pygraphblas_amd as gb
    for target in (100, 1000, 10000, 100000, 1000000):
        k = int(round(target ** 0.5))
        n = max(16, k // 2)
        rng = np.random.default_rng(3 + target)
        a, b = random_coo(rng, n, k, np.float32), random_coo(rng, n, k, np.float32)
        rec = {"probe": "sweep", "product_entries": k * k, "operand_entries": k, "n": n}
        for route in ("1", "0"):
            os.environ["GRB_MI355X_KRON"] = route
            walls = []
            for rep in range(args.reps + 1):                        # the first repetition is the warm-up
                A = gb.Matrix.from_arrays(*a, n, n, gb.FP32)        # host mirror only: the device route uploads inside the call
                B = gb.Matrix.from_arrays(*b, n, n, gb.FP32)
                gb.lib.GrBX_device_synchronize()
                t0 = time.perf_counter()
                K = A.kronecker(B)
                gb.lib.GrBX_device_synchronize()
                walls.append((time.perf_counter() - t0) * 1e3)
                assert route == "0" or gb.last_kernel_plan().startswith("kronecker<")      # (the host route leaves the plan string alone)
                del A, B, K
            rec["device_wall_ms_with_upload" if route == "1" else "host_wall_ms"] = round(float(np.median(walls[1:])), 4)
        rec["device_wins"] = rec["device_wall_ms_with_upload"] < rec["host_wall_ms"]
        emit(args.out, rec)
    os.environ.pop("GRB_MI355X_KRON", None)


def plain_store_GBps(nbytes):
    """A torch fill of `nbytes`: the `write (fill)` row of tools/membw_probe.py at this size."""
    import torch
    y = torch.empty(nbytes // 4, device=torch.device("cuda", 0), dtype=torch.float32)
    for _ in range(3):
        y.fill_(1.0)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(10):
        y.fill_(1.0)
    e.record(); torch.cuda.synchronize()
    ms = s.elapsed_time(e) / 10
    del y
    torch.cuda.empty_cache()
    return nbytes / ms / 1e6


def big(args):
    import pygraphblas_amd as gb
    lib = gb.lib
    os.environ["GRB_MI355X_KRON_TIME"] = "1"
    os.environ.pop("GRB_MI355X_KRON", None)                         # default routing: HBM-only operands take the device route by themselves
    for n, k in ((4096, 8000), (8192, 22400)):
        for t, dt in ((gb.FP32, np.float32), (gb.FP64, np.float64)):
            rng = np.random.default_rng(11)
            mats = []
            for _ in range(2):
                I, J, X = random_coo(rng, n, k, dt)
                rp = np.zeros(n + 1, np.int64); np.add.at(rp, I.astype(np.int64) + 1, 1)
                mats.append(gb.Matrix.from_csr(t, n, n, np.cumsum(rp).astype(np.uint32), J.astype(np.uint32), X))      # HBM only
            A, B = mats
            fills, calls = [], []
            for rep in range(args.reps + 1):                        # the first repetition is the warm-up (code object, pool)
                lib.GrBX_device_synchronize()
                lib.GrBX_timer_start()
                K = A.kronecker(B)
                ms = C.c_float(0); lib.GrBX_timer_stop(C.byref(ms))
                fm = C.c_float(0); lib.GrBX_kron_fill_ms(C.byref(fm))
                plan = gb.last_kernel_plan()
                nnz = int(K.nvals)
                del K
                fills.append(fm.value); calls.append(ms.value)
            assert plan.startswith("kronecker<") and nnz == k * k
            ts = np.dtype(dt).itemsize
            stored = nnz * (4 + ts)
            fill_ms, call_ms = float(np.median(fills[1:])), float(np.median(calls[1:]))
            lib.GrBX_device_synchronize()
            emit(args.out, {"probe": "big", "type": t.__name__, "n": n, "operand_entries": k, "product_entries": nnz, "stored_bytes": stored,
                            "fill_kernel_ms": round(fill_ms, 4), "fill_store_GBps": round(stored / fill_ms / 1e6, 1), "whole_call_event_ms": round(call_ms, 4),
                            "plain_store_stream_GBps_same_bytes": round(plain_store_GBps(stored), 1), "plan": plan})
            del A, B, mats


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="sweep")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kron_probe.jsonl"))
    args = ap.parse_args()
    import pygraphblas_amd as gb
    if not gb.device_info()["ok"]:
        sys.exit("kron_probe.py measures on the GPU: no HIP device")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    {"sweep": sweep, "big": big}[args.what](args)
