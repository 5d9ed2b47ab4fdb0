#!/usr/bin/env python3
"""Measurement harness: a user-defined semiring (GrBX_Semiring_new_user, grb_usersr.cpp) against the built-in semiring that computes the same thing, same
binary, same operands.  The built-in routes are the parent commit's code, unchanged: they are the yardstick; no ratio is required of the user route.

  --what rows     R-MAT-20 FP64 matrix that lives in HBM, a full operand vector: `A.mxv(v, user x + y / x * y)` against `A.mxv(v, FP64.PLUS_TIMES)`.
  --what product  R-MAT-16: `A.mxm(A, user semiring)` against `A.mxm(A, FP64.PLUS_TIMES)` in the built-in product's deterministic mode
                  (GRB_MI355X_DETERMINISTIC=1 — set by this script before the library is loaded: the user route adds in a fixed order, so that is its peer).
  --what first    the first call of a process with a user semiring, as wall time of the call: with an empty code-object cache (hipRTC compiles) and with
                  the cache of the run before (the code object is read from the disk).  Each in a fresh child process.
HIP-event time of the whole call, the median of --reps calls after a warm-up.  One JSON line per measurement is appended to --out (default
profiles/usersr_probe.jsonl).  Run each --what as its own command under `timeout`."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
from userop_probe import emit, rmat, timed


def user_plus(x, y):
    return x + y


def user_times(x, y):
    return x * y


def semiring(gb):
    add, mul = gb.binary_op(gb.FP64)(user_plus), gb.binary_op(gb.FP64)(user_times)
    mon = gb.FP64.new_monoid(add, 0.0)
    return gb.FP64.new_semiring(mon, mul), (add, mul, mon)


def rows(args):
    import pygraphblas_amd as gb
    scale = args.scale or 20
    A = rmat(gb, scale, 42)
    n = 1 << scale
    v = gb.Vector.from_arrays(np.arange(n, dtype=np.uint64), np.random.default_rng(7).random(n), n, gb.FP64)
    sr, _keep = semiring(gb)
    u_ms, u_first, nv = timed(gb.lib, lambda: A.mxv(v, sr), args.reps)
    plan = gb.last_kernel_plan()
    b_ms, _f, nv2 = timed(gb.lib, lambda: A.mxv(v, gb.FP64.PLUS_TIMES), args.reps)
    assert nv == nv2 and plan.startswith("usersr<add=user_plus,mul=user_times,type=GrB_FP64,kind=mxv>"), (nv, nv2, plan)
    emit(args.out, {"probe": "rows", "operation": "mxv", "scale": scale, "type": "FP64", "entries_A": int(A.nvals), "entries_out": int(nv), "user_ms": round(u_ms, 4),
                    "builtin_PLUS_TIMES_ms": round(b_ms, 4), "user_over_builtin": round(u_ms / b_ms, 3), "user_first_call_event_ms": round(u_first, 3), "plan": plan,
                    "builtin_plan": gb.last_kernel_plan()})


def product(args):
    import pygraphblas_amd as gb
    scale = args.scale or 16
    A = rmat(gb, scale, 42)
    sr, _keep = semiring(gb)
    u_ms, u_first, nv = timed(gb.lib, lambda: A.mxm(A, sr), args.reps)
    plan = gb.last_kernel_plan()
    b_ms, _f, nv2 = timed(gb.lib, lambda: A.mxm(A, gb.FP64.PLUS_TIMES), args.reps)
    assert nv == nv2 and plan.startswith("usersr<add=user_plus,mul=user_times,type=GrB_FP64,kind=mxm>"), (nv, nv2, plan)
    emit(args.out, {"probe": "product", "operation": "A @ A", "scale": scale, "type": "FP64", "entries_A": int(A.nvals), "entries_out": int(nv), "user_ms": round(u_ms, 4),
                    "builtin_PLUS_TIMES_deterministic_ms": round(b_ms, 4), "user_over_builtin": round(u_ms / b_ms, 3), "user_first_call_event_ms": round(u_first, 3),
                    "plan": plan[:200], "builtin_plan": gb.last_kernel_plan()[:200]})


_CHILD = r"""
import ctypes as C, json, sys, time
sys.path.insert(0, {root!r}); sys.path.insert(0, {tools!r})
import pygraphblas_amd as gb
import usersr_probe as P
A = gb.Matrix.from_lists([0, 1, 2], [1, 2, 0], [1.0, 2.0, 3.0])
v = gb.Vector.from_lists([0, 1, 2], [1.0, 2.0, 3.0])
B = A.mxv(v, gb.FP64.PLUS_TIMES); B2 = A.mxm(A, gb.FP64.PLUS_TIMES)      # the device is initialised and the pool is warm: what is timed below is the semiring's own first use
sr, keep = P.semiring(gb)
out = {{}}
for name, call in (("mxv", lambda: A.mxv(v, sr)), ("mxm", lambda: A.mxm(A, sr))):
    gb.lib.GrBX_device_synchronize()
    t0 = time.perf_counter()
    R = call()
    gb.lib.GrBX_device_synchronize()
    out[name + "_first_call_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
c, d, l = C.c_uint64(), C.c_uint64(), C.c_uint64()
gb.lib.GrBX_userop_stats(C.byref(c), C.byref(d), C.byref(l))
out.update({{"compiled": c.value, "loaded_from_disk": d.value}})
print(json.dumps(out))
"""


def first(args):
    cache = tempfile.mkdtemp(prefix="grb_usersr_probe_")
    env = dict(os.environ, GRB_MI355X_CACHE_DIR=cache)
    code = _CHILD.format(root=ROOT, tools=os.path.join(ROOT, "tools"))
    for label in ("cold (empty code-object cache: hipRTC compiles)", "warm disk cache (code object read back)"):
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.exit(r.stderr)
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        rec.update({"probe": "first", "cache": label})
        emit(args.out, rec)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="rows")
    ap.add_argument("--scale", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "usersr_probe.jsonl"))
    args = ap.parse_args()
    if args.what == "product":
        os.environ["GRB_MI355X_DETERMINISTIC"] = "1"          # (read per call by the built-in product; the user route does not look at it)
    import pygraphblas_amd as gb
    if not gb.device_info()["ok"]:
        sys.exit("usersr_probe.py measures on the GPU: no HIP device")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    {"rows": rows, "product": product, "first": first}[args.what](args)
