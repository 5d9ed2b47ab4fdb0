#!/usr/bin/env python3
"""Measurement harness: a user-defined operator (pygraphblas_amd/userop.py, grb_userop.cpp) against the built-in operator that computes the same thing,
same binary, same operands.  The built-in operator of the parent commit is the yardstick; no ratio is required of the user route.

  --what warm    R-MAT FP64 matrices that live in HBM: `A.eadd(B, user x + y)` against `A.eadd(B, FP64.PLUS)` and `A.apply(user -x)` against
                 `A.apply(FP64.AINV)`; HIP-event time of the whole call, the median of --reps calls after a warm-up (the second call onwards).
  --what first   the first call of a process with a user operator, as wall time of the call: with an empty code-object cache (the kernel is compiled
                 with hipRTC) and with the cache of the run before (the code object is read from the disk).  Each in a fresh child process.
  --what select  user-defined select operators: `A.select(user x > v, t)` against `A.select(GxB_GT_THUNK, t)` and `A.select(user j <= i)` against
                 `A.select(GxB_TRIL)` as in `warm`, then the first call of a process (empty / warm code-object cache) as in `first`.
One JSON line per measurement is appended to --out (default profiles/userop_probe.jsonl; profiles/userselect_probe.jsonl for --what select).  Run each
--what as its own command under `timeout`."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def user_plus(x, y):
    return x + y


def user_ainv(x):
    return -x


def user_gt(i, j, x, v):
    return x > v


def user_tril(i, j, x, v):
    return j <= i


def emit(out, rec):
    print(json.dumps(rec), flush=True)
    with open(out, "a") as f:
        f.write(json.dumps(rec) + "\n")


def rmat(gb, scale, seed):
    from pygraphblas_amd import rmat as R
    rp, ci = R.csr_numpy(scale, seed=seed)
    x = np.random.default_rng(seed).random(len(ci))
    return gb.Matrix.from_csr(gb.FP64, 1 << scale, 1 << scale, rp, ci, x)          # HBM only


def timed(lib, fn, reps):
    ms_all = []
    for _ in range(reps + 1):                                     # the first repetition is the warm-up (code object, pool)
        lib.GrBX_device_synchronize()
        lib.GrBX_timer_start()
        r = fn()
        ms = C.c_float(0); lib.GrBX_timer_stop(C.byref(ms))
        nv = r.nvals
        del r
        ms_all.append(ms.value)
    return float(np.median(ms_all[1:])), ms_all[0], nv


def warm(args):
    import pygraphblas_amd as gb
    lib = gb.lib
    A, B = rmat(gb, args.scale, 42), rmat(gb, args.scale, 43)
    plus, ainv = gb.binary_op(gb.FP64)(user_plus), gb.unary_op(gb.FP64)(user_ainv)
    u_ms, u_first, nv = timed(lib, lambda: A.eadd(B, plus), args.reps)
    plan = gb.last_kernel_plan()
    b_ms, _b_first, nv2 = timed(lib, lambda: A.eadd(B, gb.FP64.PLUS), args.reps)
    assert nv == nv2 and plan.startswith("userop<name=user_plus,kind=eadd")
    emit(args.out, {"probe": "warm", "operation": "eWiseAdd", "scale": args.scale, "type": "FP64", "entries_A": int(A.nvals), "entries_B": int(B.nvals), "entries_out": int(nv),
                    "user_ms": round(u_ms, 4), "builtin_PLUS_ms": round(b_ms, 4), "user_over_builtin": round(u_ms / b_ms, 3), "user_first_call_event_ms": round(u_first, 3), "plan": plan})
    u_ms, u_first, nv = timed(lib, lambda: A.apply(ainv), args.reps)
    plan = gb.last_kernel_plan()
    b_ms, _b_first, nv2 = timed(lib, lambda: A.apply(gb.FP64.AINV), args.reps)
    assert nv == nv2 and plan.startswith("userop<name=user_ainv,kind=apply")
    emit(args.out, {"probe": "warm", "operation": "apply", "scale": args.scale, "type": "FP64", "entries": int(nv), "user_ms": round(u_ms, 4), "builtin_AINV_ms": round(b_ms, 4),
                    "user_over_builtin": round(u_ms / b_ms, 3), "user_first_call_event_ms": round(u_first, 3), "plan": plan})


_CHILD = r"""
import ctypes as C, json, sys, time
sys.path.insert(0, {root!r}); sys.path.insert(0, {tools!r})
import pygraphblas_amd as gb
import userop_probe as P
A = gb.Matrix.from_lists([0, 1, 2], [1, 2, 0], [1.0, 2.0, 3.0])
B = A.apply(gb.FP64.ABS)                       # the device is initialised and the pool is warm: what is timed below is the operator's own first use
plus = gb.binary_op(gb.FP64)(P.user_plus)
gb.lib.GrBX_device_synchronize()
t0 = time.perf_counter()
R = A.eadd(B, plus)
gb.lib.GrBX_device_synchronize()
ms = (time.perf_counter() - t0) * 1e3
c, d, l = C.c_uint64(), C.c_uint64(), C.c_uint64()
gb.lib.GrBX_userop_stats(C.byref(c), C.byref(d), C.byref(l))
print(json.dumps({{"first_call_wall_ms": round(ms, 3), "compiled": c.value, "loaded_from_disk": d.value}}))
"""


def first(args):
    cache = tempfile.mkdtemp(prefix="grb_userop_probe_")
    env = dict(os.environ, GRB_MI355X_CACHE_DIR=cache)
    code = _CHILD.format(root=ROOT, tools=os.path.join(ROOT, "tools"))
    for label in ("cold (empty code-object cache: hipRTC compiles)", "warm disk cache (code object read back)"):
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.exit(r.stderr)
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        rec.update({"probe": "first", "cache": label})
        emit(args.out, rec)


_SELECT_CHILD = r"""
import ctypes as C, json, sys, time
sys.path.insert(0, {root!r}); sys.path.insert(0, {tools!r})
import pygraphblas_amd as gb
import userop_probe as P
A = gb.Matrix.from_lists([0, 1, 2], [1, 2, 0], [1.0, 2.0, 3.0])
B = A.select(">", 1.5)                         # the device is initialised and the pool is warm: what is timed below is the operator's own first use
gt = gb.select_op(gb.FP64)(P.user_gt)
gb.lib.GrBX_device_synchronize()
t0 = time.perf_counter()
R = A.select(gt, 1.5)
gb.lib.GrBX_device_synchronize()
ms = (time.perf_counter() - t0) * 1e3
assert R.nvals == B.nvals == 2
c, d, l = C.c_uint64(), C.c_uint64(), C.c_uint64()
gb.lib.GrBX_userop_stats(C.byref(c), C.byref(d), C.byref(l))
print(json.dumps({{"first_call_wall_ms": round(ms, 3), "compiled": c.value, "loaded_from_disk": d.value}}))
"""


def select(args):
    import pygraphblas_amd as gb
    lib = gb.lib
    A = rmat(gb, args.scale, 42)
    gt, tril = gb.select_op(gb.FP64)(user_gt), gb.select_op(gb.FP64)(user_tril)
    for name, user, built in (("x > v against GxB_GT_THUNK", lambda: A.select(gt, 0.5), lambda: A.select(">", 0.5)),
                              ("j <= i against GxB_TRIL", lambda: A.select(tril), lambda: A.select("TRIL"))):
        u_ms, u_first, nv = timed(lib, user, args.reps)
        plan = gb.last_kernel_plan()
        b_ms, _b_first, nv2 = timed(lib, built, args.reps)
        assert nv == nv2 and plan.startswith("userselect<name=user_"), (nv, nv2, plan)
        emit(args.out, {"probe": "select", "operation": name, "scale": args.scale, "type": "FP64", "entries": int(A.nvals), "entries_out": int(nv), "user_ms": round(u_ms, 4),
                        "builtin_ms": round(b_ms, 4), "user_over_builtin": round(u_ms / b_ms, 3), "user_first_call_event_ms": round(u_first, 3), "plan": plan})
    cache = tempfile.mkdtemp(prefix="grb_userselect_probe_")
    env = dict(os.environ, GRB_MI355X_CACHE_DIR=cache)
    code = _SELECT_CHILD.format(root=ROOT, tools=os.path.join(ROOT, "tools"))
    for label in ("cold (empty code-object cache: hipRTC compiles)", "warm disk cache (code object read back)"):
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.exit(r.stderr)
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        rec.update({"probe": "select first", "cache": label})
        emit(args.out, rec)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="warm")
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "userselect_probe.jsonl" if args.what == "select" else "userop_probe.jsonl")
    import pygraphblas_amd as gb
    if not gb.device_info()["ok"]:
        sys.exit("userop_probe.py measures on the GPU: no HIP device")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    {"warm": warm, "first": first, "select": select}[args.what](args)
