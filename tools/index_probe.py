#!/usr/bin/env python3
"""Measurement harness: an index list that lies in HBM (a GPU tensor through GrBX_*_at, parsed by grb_index.hip) against the SAME call with the same list in a
numpy array — the route every call took before device lists existed: a serial scan of the list on the host and an upload of 4 bytes per index.

  v.extract(I), A.extract_matrix(I, I), v.assign(u, I) on R-MAT-20 (FP32), operands living in HBM only, |I| from 1e3 to 1e7:
    shuffled      a random permutation's prefix (beyond n: sampled with repeats, extract of the vector only)
    increasing    a sorted sample
    select        the positions a `select` keeps, taken with to_tensors(values=False) — the list is born in HBM
  Wall clock around a device synchronisation, the median of --reps after a warm-up.  Lists longer than n are measured for v.extract only (the matrix result
  would grow with |I|^2 under repeats, and assign takes no repeats on the device route).
  parse         the parse kernel alone (GrBX_index_parse: status word read back) against a Tensor.copy_ that moves the same 12 bytes per index.
No dispatch decision hangs on these numbers.  One JSON line per measurement is appended to --out (default profiles/index_probe.jsonl)."""
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


def wall_ms(gb, call, reps):
    import torch
    walls = []
    for rep in range(reps + 1):                                     # the first repetition is the warm-up
        gb.lib.GrBX_device_synchronize(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = call()
        gb.lib.GrBX_device_synchronize(); torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
        del r
    return round(float(np.median(walls[1:])), 4)


def main(args):
    import torch
    import pygraphblas_amd as gb
    from pygraphblas_amd import rmat
    dev = torch.device("cuda", 0)
    scale = args.scale
    n = 1 << scale
    rowptr, col = rmat.csr_torch(scale, dev, seed=42)
    nnz = col.numel()
    vals = rmat.values_torch(nnz, dev, seed=43, dtype=torch.float32)
    A = gb.Matrix.from_csr(gb.FP32, n, n, rowptr.data_ptr(), col.data_ptr(), (vals.data_ptr(), nnz), device=True)
    rng = np.random.default_rng(5)
    v = gb.Vector.from_dense_array(rng.random(n).astype(np.float32), gb.FP32)
    sel_src = gb.Vector.from_dense_array(rng.random(n).astype(np.float32), gb.FP32)
    perm = rng.permutation(n)
    for size in [int(float(s)) for s in args.sizes.split(",")]:
        lists = {}
        if size <= n:
            lists["shuffled"] = perm[:size].astype(np.int64)
            lists["increasing"] = np.sort(perm[:size]).astype(np.int64)
            (sel,) = sel_src.select("<", size / n).to_tensors(values=False)      # about `size` positions, increasing, never on the host
            lists["select"] = sel
        else:
            lists["shuffled"] = rng.integers(0, n, size).astype(np.int64)
        for kind, L in lists.items():
            It = L if torch.is_tensor(L) else torch.from_numpy(L).to(dev)
            Ih = It.cpu().numpy().view(np.uint64)
            k = int(It.numel())
            ops = {"v.extract(I)": lambda I: v.extract(I)}
            if size <= n:
                u = gb.Vector.from_dense_array(rng.random(k).astype(np.float32), gb.FP32)
                w = gb.Vector.from_dense_array(rng.random(n).astype(np.float32), gb.FP32)
                ops["A.extract_matrix(I, I)"] = lambda I: A.extract_matrix(I, I)
                ops["v.assign(u, I)"] = lambda I: w.assign(u, I)
            for name, op in ops.items():
                dev_ms = wall_ms(gb, lambda: op(It), args.reps)
                plan = gb.last_kernel_plan()
                host_ms = wall_ms(gb, lambda: op(Ih), args.reps)
                emit(args.out, {"probe": "index", "scale": scale, "op": name, "list": kind, "indices": k, "device_list_wall_ms": dev_ms, "host_list_wall_ms": host_ms,
                                "host_over_device": round(host_ms / dev_ms, 2), "plan": plan})
        # the parse alone against a copy of the same bytes: 8 read + 4 written per index
        It = torch.from_numpy(lists["shuffled"]).to(dev)
        k = int(It.numel())
        inc = C.c_int(0)
        parse_ms = wall_ms(gb, lambda: gb.lib.GrBX_index_parse(C.c_void_p(It.data_ptr()), C.c_uint64(k), C.c_uint64(n), C.byref(inc)), args.reps)
        src, dst = torch.empty(k * 6, dtype=torch.uint8, device=dev), torch.empty(k * 6, dtype=torch.uint8, device=dev)      # 6 bytes read + 6 written = 12 per index
        copy_ms = wall_ms(gb, lambda: dst.copy_(src), args.reps)
        emit(args.out, {"probe": "parse", "indices": k, "parse_wall_ms": parse_ms, "copy_12_bytes_per_index_wall_ms": copy_ms, "parse_GBps": round(k * 12 / parse_ms / 1e6, 1)})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--sizes", default="1e3,1e4,1e5,1e6,1e7")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_probe.jsonl"))
    args = ap.parse_args()
    import pygraphblas_amd as gb
    if not gb.device_info()["ok"]:
        sys.exit("index_probe.py measures on the GPU: no HIP device")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    main(args)
