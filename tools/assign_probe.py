#!/usr/bin/env python3
"""Measurement harness: index-list assign, device route (grb_assign.hip) against the host route of grb_assign_ops.cpp (GRB_MI355X_ASSIGN=0: what
every call took before the device route existed), same binary, process-fresh inputs.

  --what big     R-MAT at --scales (default 20,22), device-only C, the four selections of tests/test_assign_gpu.py: S = C[I, I] is cut out, scaled
                 and written back with C[I, I] = S.  HIP-event and wall time per call after a warm-up, and the whole call's rate against
                 (nnz(C) + nnz(S)) (4 + sizeof T) 2 bytes (C and the block read once, the result written once).  The host route runs in a child
                 process under --host-limit seconds ("did not finish" is a result); after a child that ended abnormally nothing more is started.
  --what sweep   the threshold of GrB_Matrix_assign's dispatch: uniform random matrices of 1e3 .. 1e6 entries whose only valid image is the HOST mirror,
                 a block holding a quarter as many entries written to C[I, I] for half of the vertices; one call on each route, upload included,
                 median over fresh matrices.  Where the host's general path walks |I| x |J| positions for minutes, ONE host call runs in a child
                 process under --sweep-host-limit seconds.
  --what lines   the same for GrB_Row_assign, GrB_Col_assign (`M[i] = v`, `M[:, j] = v`, and a shuffled list under a mask) and GrB_Vector_assign.
One JSON line per measurement is appended to --out (default profiles/assign_probe.jsonl).  Run each --what as its own command under `timeout`."""
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

SELECTIONS = ["range", "sorted sample", "shuffled", "hubs and neighbours"]


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
    if which == "shuffled":
        sh = rng.permutation(sample)
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
        call()
    ms = C.c_float(0)
    lib.GrBX_timer_stop(C.byref(ms))
    lib.GrBX_device_synchronize()
    return ms.value / reps, (time.perf_counter() - t0) * 1e3 / reps


def big(args):
    import pygraphblas_amd as gb
    for scale in [int(s) for s in args.scales.split(",")]:
        Cm, rp, col, nnz = build_rmat(gb, scale)
        n = 1 << scale
        for which in SELECTIONS:
            arg, idx = selection(which, n, rp, col)
            os.environ["GRB_MI355X_ASSIGN"] = "1"
            S = Cm.extract_matrix(arg, arg).apply_second(gb.FP32.TIMES, 2.0)
            Cm.assign_matrix(S, arg, arg)                           # warm-up: code objects, pool (the pattern of C does not change)
            ev, wall = timed(gb, lambda: Cm.assign_matrix(S, arg, arg), args.reps)
            plan = gb.last_kernel_plan()
            block = int(S.nvals)
            moved = (nnz + block) * (4 + 4) * 2
            emit(args.out, {"probe": "big", "route": "device", "scale": scale, "nnz": nnz, "selection": which, "rows": int(len(idx)), "block_entries": block,
                            "event_ms": round(ev, 4), "wall_ms": round(wall, 4), "bytes": moved, "whole_call_GBps": round(moved / ev / 1e6, 1), "plan": plan})
            del S
        del Cm
        for which in args.host_selections.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--what", "host-child", "--scales", str(scale), "--selection", which, "--out", args.out]
            t0 = time.perf_counter()
            try:
                subprocess.run(cmd, timeout=args.host_limit, check=True)     # a fresh child process: its own device context, nothing of this one's is replaced
            except subprocess.TimeoutExpired:                        # (the child was killed inside the host route's CPU loop, not in a kernel: the next child may start)
                emit(args.out, {"probe": "big", "route": "host", "scale": scale, "selection": which, "result": f"did not finish in {args.host_limit} s"})
            except subprocess.CalledProcessError as e:
                emit(args.out, {"probe": "big", "route": "host", "scale": scale, "selection": which, "result": f"failed with exit status {e.returncode} after {time.perf_counter() - t0:.0f} s"})
                sys.exit(1)                                           # nothing more is started after a child that ended abnormally


def host_child(args):
    import pygraphblas_amd as gb
    scale = int(args.scales)
    Cm, rp, col, nnz = build_rmat(gb, scale)
    arg, idx = selection(args.selection, 1 << scale, rp, col)
    S = Cm.extract_matrix(arg, arg).apply_second(gb.FP32.TIMES, 2.0)
    os.environ["GRB_MI355X_ASSIGN"] = "0"
    t0 = time.perf_counter()
    Cm.assign_matrix(S, arg, arg)                                   # the first call pays the download of C and S; a second one would not
    first = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    Cm.assign_matrix(S, arg, arg)
    second = (time.perf_counter() - t0) * 1e3
    emit(args.out, {"probe": "big", "route": "host", "scale": scale, "nnz": nnz, "selection": args.selection, "rows": int(len(idx)), "block_entries": int(S.nvals),
                    "wall_ms_first_call_with_download": round(first, 2), "wall_ms_second_call": round(second, 2)})


def sweep_inputs(target, seed=3):
    rng = np.random.default_rng(seed + target)
    n = max(64, target // 16)
    flat = np.sort(rng.choice(n * n, size=target, replace=False))
    I, J = np.divmod(flat, n)
    I, J, X = I.astype(np.uint64), J.astype(np.uint64), rng.random(target).astype(np.float32)
    inc = np.sort(rng.choice(n, size=n // 2, replace=False))
    m = len(inc)
    bflat = np.sort(rng.choice(m * m, size=max(1, target // 4), replace=False))
    BI, BJ = np.divmod(bflat, m)
    BI, BJ, BX = BI.astype(np.uint64), BJ.astype(np.uint64), rng.random(len(bflat)).astype(np.float32)
    return n, m, (I, J, X), (BI, BJ, BX), {"increasing list": inc, "shuffled list": rng.permutation(inc)}


def sweep_host_child(args):
    import pygraphblas_amd as gb
    n, m, (I, J, X), (BI, BJ, BX), sels = sweep_inputs(args.entries)
    os.environ["GRB_MI355X_ASSIGN"] = "0"
    Cm = gb.Matrix.from_arrays(I, J, X, n, n, gb.FP32)
    B = gb.Matrix.from_arrays(BI, BJ, BX, m, m, gb.FP32)
    M = gb.Matrix.from_arrays(I[::2], J[::2], np.ones(len(I[::2]), np.bool_), n, n, gb.BOOL) if args.masked else None
    t0 = time.perf_counter()
    Cm.assign_matrix(B, sels[args.selection], sels[args.selection], mask=M)
    print(round((time.perf_counter() - t0) * 1e3, 4))


def lines(args):
    """GrB_Row_assign / GrB_Col_assign / GrB_Vector_assign on host-resident containers, one call per route, uploads included."""
    import pygraphblas_amd as gb
    for target in (10000, 100000, 1000000, 3000000):
        n, m, (I, J, X), _b, sels = sweep_inputs(target)
        rng = np.random.default_rng(5)
        vi = np.arange(0, n, 3, dtype=np.uint64)
        v = (vi, rng.random(len(vi)).astype(np.float32))
        idx = sels["shuffled list"]
        ui = np.arange(0, m, 2, dtype=np.uint64)
        u = (ui, rng.random(len(ui)).astype(np.float32))
        mi = np.arange(0, n, 2, dtype=np.uint64)
        shapes = {"row, all": lambda Cm, V, U, M: Cm.assign_row(n // 3, V), "col, all": lambda Cm, V, U, M: Cm.assign_col(n // 3, V),
                  "row, shuffled list, mask": lambda Cm, V, U, M: Cm.assign_row(n // 3, U, idx, mask=M), "col, shuffled list, mask": lambda Cm, V, U, M: Cm.assign_col(n // 3, U, idx, mask=M)}
        for name, call in shapes.items():
            rec = {"probe": "lines", "entries": target, "n": n, "shape": name}
            for route in ("1", "0"):
                os.environ["GRB_MI355X_ASSIGN"] = route
                walls = []
                for rep in range(args.reps + 1):
                    Cm = gb.Matrix.from_arrays(I, J, X, n, n, gb.FP32)
                    V = gb.Vector.from_arrays(v[0], v[1], n, gb.FP32); U = gb.Vector.from_arrays(u[0], u[1], m, gb.FP32)
                    M = gb.Vector.from_arrays(mi, np.ones(len(mi), np.bool_), n, gb.BOOL)
                    gb.lib.GrBX_device_synchronize()
                    t0 = time.perf_counter()
                    call(Cm, V, U, M)
                    gb.lib.GrBX_device_synchronize()
                    walls.append((time.perf_counter() - t0) * 1e3)
                    del Cm, V, U, M
                rec["device_wall_ms_with_upload" if route == "1" else "host_wall_ms"] = round(float(np.median(walls[1:])), 4)
            emit(args.out, rec)
    for size in (1000, 10000, 100000, 1000000):
        rng = np.random.default_rng(6)
        wi = np.arange(0, size, 2, dtype=np.uint64); wx = rng.random(len(wi)).astype(np.float32)
        for name in ("all", "shuffled list"):
            idx = None if name == "all" else rng.permutation(size)[: size // 2]
            k = size if idx is None else len(idx)
            ui = np.arange(0, k, 2, dtype=np.uint64); ux = rng.random(len(ui)).astype(np.float32)
            rec = {"probe": "lines", "entries": int(len(wi)), "n": size, "shape": "vector, " + name}
            for route in ("1", "0"):
                os.environ["GRB_MI355X_ASSIGN"] = route
                walls = []
                for rep in range(args.reps + 1):
                    w = gb.Vector.from_arrays(wi, wx, size, gb.FP32); U = gb.Vector.from_arrays(ui, ux, k, gb.FP32)
                    gb.lib.GrBX_device_synchronize()
                    t0 = time.perf_counter()
                    w.assign(U, idx)
                    gb.lib.GrBX_device_synchronize()
                    walls.append((time.perf_counter() - t0) * 1e3)
                    del w, U
                rec["device_wall_ms_with_upload" if route == "1" else "host_wall_ms"] = round(float(np.median(walls[1:])), 4)
            emit(args.out, rec)


def sweep(args):
    import pygraphblas_amd as gb
    for target in (1000, 3000, 10000, 30000, 100000, 1000000):
        n, m, (I, J, X), (BI, BJ, BX), sels = sweep_inputs(target)
        for name, idx in sels.items():
            for masked in (False, True):
                rec = {"probe": "sweep", "entries": target, "block_entries": int(len(BI)), "n": n, "selection": name, "mask": masked}
                for route in ("1", "0"):
                    if route == "0" and (masked or name != "increasing list") and target > 30000:
                        # the host's general path walks |I| x |J| positions: one call, in a child under a time limit (killed in CPU code: nothing on the GPU is cut short)
                        cmd = [sys.executable, os.path.abspath(__file__), "--what", "sweep-host-child", "--entries", str(target), "--selection", name] + (["--masked"] if masked else [])
                        try:
                            r = subprocess.run(cmd, timeout=args.sweep_host_limit, check=True, capture_output=True, text=True)
                            rec["host_wall_ms"] = float(r.stdout.strip().splitlines()[-1])
                        except subprocess.TimeoutExpired:
                            rec["host_wall_ms"] = f"did not finish in {args.sweep_host_limit} s"
                        continue
                    os.environ["GRB_MI355X_ASSIGN"] = route
                    walls = []
                    for rep in range(args.reps + 1):                # the first repetition is the warm-up
                        Cm = gb.Matrix.from_arrays(I, J, X, n, n, gb.FP32)     # host mirror only: the device route uploads inside the call
                        B = gb.Matrix.from_arrays(BI, BJ, BX, m, m, gb.FP32)
                        M = gb.Matrix.from_arrays(I[::2], J[::2], np.ones(len(I[::2]), np.bool_), n, n, gb.BOOL) if masked else None
                        gb.lib.GrBX_device_synchronize()
                        t0 = time.perf_counter()
                        Cm.assign_matrix(B, idx, idx, mask=M)
                        gb.lib.GrBX_device_synchronize()
                        walls.append((time.perf_counter() - t0) * 1e3)
                        del Cm, B, M
                    rec["device_wall_ms_with_upload" if route == "1" else "host_wall_ms"] = round(float(np.median(walls[1:])), 4)
                emit(args.out, rec)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="sweep")
    ap.add_argument("--scales", default="20,22")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-limit", type=int, default=60)
    ap.add_argument("--sweep-host-limit", type=int, default=20)
    ap.add_argument("--entries", type=int, default=100000)
    ap.add_argument("--masked", action="store_true")
    ap.add_argument("--host-selections", default="range,sorted sample,shuffled,hubs and neighbours")
    ap.add_argument("--selection", default="range")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assign_probe.jsonl"))
    args = ap.parse_args()
    if args.what == "host-child":
        host_child(args)
    elif args.what == "sweep-host-child":
        sweep_host_child(args)
    else:
        import pygraphblas_amd as gb
        if not gb.device_info()["ok"]:
            sys.exit("assign_probe.py measures on the GPU: no HIP device")
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        {"sweep": sweep, "lines": lines, "big": big}[args.what](args)
