#!/usr/bin/env python3
"""Measurement harness: index-list extract, device route (grb_extract.hip) against the host route of grb_extract_ops.cpp (GRB_MI355X_EXTRACT=0: what
every call took before the device route existed), same binary, process-fresh inputs.

  --what big     R-MAT at --scales (default 20,22), device-only operand, the four selections of tests/test_extract_gpu.py: HIP-event and wall
                 time per call after a warm-up, and the whole call's rate against nnz(selected rows) (4 + sizeof T) 2 bytes (count + fill passes).
                 The host route runs in a child process under --host-limit seconds ("did not finish" is a result).
  --what sweep   the threshold of the dispatch: uniform random matrices of 1e3 .. 1e6 entries whose only valid image is the HOST mirror; one call on
                 each route, upload included, median over fresh matrices.
One JSON line per measurement is appended to --out (default profiles/extract_probe.jsonl)."""
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

SELECTIONS = ["range", "sorted sample", "shuffled with repeats", "hubs and neighbours"]


def emit(out, rec):
    print(json.dumps(rec), flush=True)
    with open(out, "a") as f:
        f.write(json.dumps(rec) + "\n")


def build_rmat(gb, scale):
    import torch
    from pygraphblas_amd import rmat
    dev = torch.device("cuda", 0)
    rowptr, col = rmat.csr_torch(scale, dev, seed=42)
    nnz = col.numel()
    vals = rmat.values_torch(nnz, dev, seed=43, dtype=torch.float32)
    A = gb.Matrix.from_csr(gb.FP32, 1 << scale, 1 << scale, rowptr.data_ptr(), col.data_ptr(), (vals.data_ptr(), nnz), device=True)
    torch.cuda.synchronize()
    return A, rowptr.cpu().numpy().astype(np.int64), col, nnz


def selection(which, n, rp, col):
    rng = np.random.default_rng(7)
    deg = np.diff(rp)
    if which == "range":
        return slice(0, n // 2 - 1), np.arange(n // 2)
    sample = np.sort(rng.choice(n, size=n // 10, replace=False))
    if which == "sorted sample":
        return sample, sample
    if which == "shuffled with repeats":
        sh = rng.permutation(sample)
        sh[rng.choice(len(sh), size=len(sh) // 100, replace=False)] = sh[0]
        return sh, sh
    hubs = np.argsort(-deg, kind="stable")[:64]
    nb = np.unique(np.concatenate([col[int(rp[h]):int(rp[h + 1])].cpu().numpy().astype(np.int64) for h in hubs[:4]] + [hubs]))
    return nb, nb


def timed(gb, call, reps):
    """(HIP-event ms, wall ms) per call, the mean over reps, after the caller's warm-up."""
    lib = gb.lib
    lib.GrBX_device_synchronize()
    t0 = time.perf_counter()
    lib.GrBX_timer_start()
    for _ in range(reps):
        r = call()
    ms = C.c_float(0)
    lib.GrBX_timer_stop(C.byref(ms))
    lib.GrBX_device_synchronize()
    return ms.value / reps, (time.perf_counter() - t0) * 1e3 / reps, r


def big(args):
    import pygraphblas_amd as gb
    for scale in [int(s) for s in args.scales.split(",")]:
        A, rp, col, nnz = build_rmat(gb, scale)
        n = 1 << scale
        for which in SELECTIONS:
            arg, idx = selection(which, n, rp, col)
            src = int(np.diff(rp)[idx].sum())
            os.environ["GRB_MI355X_EXTRACT"] = "1"
            sub = A.extract_matrix(arg, arg)                        # warm-up: code objects, pool
            ev, wall, sub = timed(gb, lambda: A.extract_matrix(arg, arg), args.reps)
            moved = src * (4 + 4) * 2
            emit(args.out, {"probe": "big", "route": "device", "scale": scale, "nnz": nnz, "selection": which, "rows": int(len(idx)), "entries_of_selected_rows": src,
                            "result_entries": int(sub.nvals), "event_ms": round(ev, 4), "wall_ms": round(wall, 4), "count_fill_bytes": moved,
                            "whole_call_GBps_of_count_fill_bytes": round(moved / ev / 1e6, 1), "plan": gb.last_kernel_plan()})
            del sub
        del A
        for which in args.host_selections.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--what", "host-child", "--scales", str(scale), "--selection", which, "--out", args.out]
            t0 = time.perf_counter()
            try:
                subprocess.run(cmd, timeout=args.host_limit, check=True)     # a fresh child process: its own device context, nothing of this one's is replaced
            except subprocess.TimeoutExpired:
                emit(args.out, {"probe": "big", "route": "host", "scale": scale, "selection": which, "result": f"did not finish in {args.host_limit} s"})
            except subprocess.CalledProcessError as e:
                emit(args.out, {"probe": "big", "route": "host", "scale": scale, "selection": which, "result": f"failed with exit status {e.returncode} after {time.perf_counter() - t0:.0f} s"})


def host_child(args):
    import pygraphblas_amd as gb
    scale = int(args.scales)
    A, rp, col, nnz = build_rmat(gb, scale)
    arg, idx = selection(args.selection, 1 << scale, rp, col)
    os.environ["GRB_MI355X_EXTRACT"] = "0"
    t0 = time.perf_counter()
    sub = A.extract_matrix(arg, arg)                                # the first call pays the download of A; a second one would not
    first = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    sub = A.extract_matrix(arg, arg)
    second = (time.perf_counter() - t0) * 1e3
    emit(args.out, {"probe": "big", "route": "host", "scale": scale, "nnz": nnz, "selection": args.selection, "rows": int(len(idx)), "result_entries": int(sub.nvals),
                    "wall_ms_first_call_with_download": round(first, 2), "wall_ms_second_call": round(second, 2)})


def sweep(args):
    import pygraphblas_amd as gb
    rng = np.random.default_rng(3)
    for target in (1000, 10000, 100000, 1000000):
        n = max(64, target // 16)
        flat = np.sort(rng.choice(n * n, size=target, replace=False))
        I, J = np.divmod(flat, n)
        I, J, X = I.astype(np.uint64), J.astype(np.uint64), rng.random(target).astype(np.float32)
        inc = np.sort(rng.choice(n, size=n // 2, replace=False))
        sels = {"increasing list": inc, "shuffled list": rng.permutation(inc)}
        for name, idx in sels.items():
            rec = {"probe": "sweep", "entries": target, "n": n, "selection": name}
            for route in ("1", "0"):
                os.environ["GRB_MI355X_EXTRACT"] = route
                walls = []
                for rep in range(args.reps + 1):                    # the first repetition is the warm-up
                    A = gb.Matrix.from_arrays(I, J, X, n, n, gb.FP32)       # host mirror only: the device route uploads it inside the call
                    gb.lib.GrBX_device_synchronize()
                    t0 = time.perf_counter()
                    sub = A.extract_matrix(idx, idx)
                    gb.lib.GrBX_device_synchronize()
                    walls.append((time.perf_counter() - t0) * 1e3)
                    del A, sub
                rec["device_wall_ms_with_upload" if route == "1" else "host_wall_ms"] = round(float(np.median(walls[1:])), 4)
            emit(args.out, rec)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="sweep,big")
    ap.add_argument("--scales", default="20,22")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-limit", type=int, default=180)
    ap.add_argument("--host-selections", default="range,shuffled with repeats")
    ap.add_argument("--selection", default="range")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extract_probe.jsonl"))
    args = ap.parse_args()
    if args.what == "host-child":
        host_child(args)
    else:
        import pygraphblas_amd as gb
        if not gb.device_info()["ok"]:
            sys.exit("extract_probe.py measures on the GPU: no HIP device")
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        for w in args.what.split(","):
            {"sweep": sweep, "big": big}[w](args)
