#!/usr/bin/env python3
"""Measurement harness: matrix scalar assign C<M>(I, J) = s, the device routes (grb_assign_scalar.hip) against the host-built block (GRB_MI355X_ASSIGN_SCALAR=0:
what every call took before the device routes existed), same binary.

  --what sweep    unmasked blocks of 1e2 .. 1e7 positions (a row range x a column range) into an FP32 matrix of 4096 x 4096 with 1e5 entries, once with
                  only its host mirror valid (the call pays the upload) and once living in HBM only.
  --what masked   C<M> = s over GrB_ALL x GrB_ALL: R-MAT at --scales (default 18,20) with M = C's pattern, and a 30 000 x 30 000 matrix with nnz(M) = 1e5.
                  The host-built block materialises every position: where that cannot fit it answers GrB_OUT_OF_MEMORY at once (recorded as such), and
                  where it would run for many seconds ONE call runs in a child process under --host-limit seconds ("did not finish" is a result); after
                  a child that ended abnormally nothing more is started.
Each configuration runs once per route: the median of --reps calls after a warm-up, on fresh containers, HIP events over the whole call and wall time.
One JSON line per measurement is appended to --out (default profiles/assign_scalar_probe.jsonl).  Run each --what as its own command under `timeout`."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ROUTES = (("device", None), ("host_block", "0"))


def emit(out, rec):
    print(json.dumps(rec), flush=True)
    with open(out, "a") as f:
        f.write(json.dumps(rec) + "\n")


def set_route(value):
    if value is None:
        os.environ.pop("GRB_MI355X_ASSIGN_SCALAR", None)
    else:
        os.environ["GRB_MI355X_ASSIGN_SCALAR"] = value


def one_call(gb, make, call):
    """(HIP-event ms, wall ms) of one call on fresh containers."""
    lib = gb.lib
    objs = make()
    lib.GrBX_device_synchronize()
    t0 = time.perf_counter()
    lib.GrBX_timer_start()
    call(*objs)
    ms = C.c_float(0)
    lib.GrBX_timer_stop(C.byref(ms))
    lib.GrBX_device_synchronize()
    return ms.value, (time.perf_counter() - t0) * 1e3


def measure(gb, make, call, reps):
    runs = [one_call(gb, make, call) for _ in range(reps + 1)][1:]      # the first is the warm-up
    return round(float(np.median([r[0] for r in runs])), 4), round(float(np.median([r[1] for r in runs])), 4)


def random_tuples(n, nnz, seed):
    rng = np.random.default_rng(seed)
    flat = np.unique(rng.integers(0, n * n, nnz, dtype=np.int64))
    I, J = np.divmod(flat, n)
    return I.astype(np.uint64), J.astype(np.uint64), rng.random(len(flat)).astype(np.float32)


def sweep(args):
    import pygraphblas_amd as gb
    n = 4096
    I, J, X = random_tuples(n, 100000, 11)
    for positions in (100, 1000, 10000, 100000, 1000000, 10000000):
        side = int(round(positions ** 0.5))
        rows, cols = slice(7, 7 + side - 1), slice(3, 3 + side - 1)
        for residency in ("host mirror", "HBM only"):
            def make():
                A = gb.Matrix.from_arrays(I, J, X, n, n, gb.FP32)
                return (A.apply_second(gb.FP32.TIMES, 1.0),) if residency == "HBM only" else (A,)      # (the result of a device operation has no host mirror)
            rec = {"probe": "sweep", "positions": side * side, "side": side, "C": residency}
            for name, value in ROUTES:
                set_route(value)
                rec[name + "_event_ms"], rec[name + "_wall_ms"] = measure(gb, make, lambda A: A.assign_scalar(2.0, rows, cols), args.reps)
                if value is None:
                    rec["plan"] = gb.last_kernel_plan()
            rec["host_over_device"] = round(rec["host_block_wall_ms"] / rec["device_wall_ms"], 2)
            emit(args.out, rec)


def rmat_inputs(gb, scale):
    import torch
    from pygraphblas_amd import rmat
    dev = torch.device("cuda", 0)
    rowptr, col = rmat.csr_torch(scale, dev, seed=42)
    nnz = col.numel()
    vals = rmat.values_torch(nnz, dev, seed=43, dtype=torch.float32)
    A = gb.Matrix.from_csr(gb.FP32, 1 << scale, 1 << scale, rowptr.data_ptr(), col.data_ptr(), (vals.data_ptr(), nnz), device=True)
    torch.cuda.synchronize()
    return A, nnz


def masked_case(gb, name):
    """(make, the matrix's dimension, nnz(M)) for one masked configuration."""
    if name.startswith("rmat"):
        base, nnz = rmat_inputs(gb, int(name[4:]))
        return (lambda: (base.dup(), base)), base.nrows, nnz
    n = 30000
    I, J, X = random_tuples(n, 100000, 12)
    MI, MJ, MX = random_tuples(n, 100000, 13)
    return (lambda: (gb.Matrix.from_arrays(I, J, X, n, n, gb.FP32), gb.Matrix.from_arrays(MI, MJ, np.ones(len(MI), np.bool_), n, n, gb.BOOL))), n, len(MI)


def masked(args):
    import pygraphblas_amd as gb
    for name in ["rmat" + s for s in args.scales.split(",")] + ["uniform30000"]:
        make, n, mnz = masked_case(gb, name)
        rec = {"probe": "masked", "case": name, "n": n, "positions": n * n, "mask_entries": int(mnz)}
        set_route(None)
        rec["device_event_ms"], rec["device_wall_ms"] = measure(gb, make, lambda A, M: A.assign_scalar(2.0, mask=M), args.reps)
        rec["plan"] = gb.last_kernel_plan()
        if n * n > 0xFFFFFFF0:
            set_route("0")
            A, M = make()
            try:
                A.assign_scalar(2.0, mask=M)
                rec["host_block"] = "ran"                             # (cannot happen: the block has more positions than the layout holds)
            except gb.base.GraphBLASException as e:
                rec["host_block"] = f"{type(e).__name__}: {e}"
            set_route(None)
        else:
            cmd = [sys.executable, os.path.abspath(__file__), "--what", "masked-host-child", "--case", name]
            t0 = time.perf_counter()
            try:
                r = subprocess.run(cmd, timeout=args.host_limit, check=True, capture_output=True, text=True)      # a fresh child process: its own device context
                rec["host_block_wall_ms"] = float(r.stdout.strip().splitlines()[-1])
            except subprocess.TimeoutExpired:                         # (killed inside the host's CPU loop or its copies, not in a kernel of ours)
                rec["host_block"] = f"did not finish in {args.host_limit} s"
            except subprocess.CalledProcessError as e:
                rec["host_block"] = f"failed with exit status {e.returncode} after {time.perf_counter() - t0:.0f} s"
                emit(args.out, rec)
                sys.exit(1)                                           # nothing more is started after a child that ended abnormally
        emit(args.out, rec)


def masked_host_child(args):
    import pygraphblas_amd as gb
    make, n, mnz = masked_case(gb, args.case)
    set_route("0")
    A, M = make()
    gb.lib.GrBX_device_synchronize()
    t0 = time.perf_counter()
    A.assign_scalar(2.0, mask=M)
    gb.lib.GrBX_device_synchronize()
    print(round((time.perf_counter() - t0) * 1e3, 4))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="sweep")
    ap.add_argument("--scales", default="18,20")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-limit", type=int, default=60)
    ap.add_argument("--case", default="uniform30000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assign_scalar_probe.jsonl"))
    args = ap.parse_args()
    if args.what == "masked-host-child":
        masked_host_child(args)
    else:
        import pygraphblas_amd as gb
        if not gb.device_info()["ok"]:
            sys.exit("assign_scalar_probe.py measures on the GPU: no HIP device")
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        {"sweep": sweep, "masked": masked}[args.what](args)
