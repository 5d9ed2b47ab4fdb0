#!/usr/bin/env python3
"""Measurement harness: element edits and resize of matrices that live in HBM only — the edit queue and its flush (grb_edit.hip) against the route every
such call took before (download, host tuples, rebuild, upload; GRB_MI355X_EDIT=0 of this build, or the parent commit running this same script: only calls
the parent has are used, `resize` through the C entry point).

  --what big     R-MAT matrices (--scales, default 20 22), FP64, HBM only, a fresh device copy per repetition:
                   pair    one insert + the next `mxv`
                   triple  4 096 mixed edits + the flush (`nvals`) + `mxv`
                   resize  to half the columns
                 and, from the same run, the whole structural flush with the edits queued beforehand and the whole resize, with the bytes/s of the CSR
                 arrays they read and write over that time (lower bounds of the stream pass's and of `csr_compact`'s own rates).
  --what sweep   1e3 .. 1e7 entries x 1 / 64 / 4 096 edits followed by an `mxv`, both routes: the table behind a size threshold.
Wall time around a device synchronisation on both routes (the host route is host work), HIP-event time beside it; the median of --reps after a warm-up.
One JSON line per measurement is appended to --out (default profiles/edit_probe.jsonl).  Run each --what as its own command under `timeout`."""
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


def measure(gb, reps, make, call, prepare=None):
    walls, events = [], []
    for rep in range(reps + 1):                                     # the first repetition is the warm-up
        operand = make()
        if prepare is not None:
            prepare(operand)                                        # outside the timed interval
        gb.lib.GrBX_device_synchronize()
        gb.lib.GrBX_timer_start()
        t0 = time.perf_counter()
        call(operand)
        gb.lib.GrBX_device_synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
        ms = C.c_float(0); gb.lib.GrBX_timer_stop(C.byref(ms)); events.append(ms.value)
        del operand
    return round(float(np.median(walls[1:])), 4), round(float(np.median(events[1:])), 4)


def mixed_edits(rng, rp, col, n, k):
    """k records: a third overwrites, a third inserts (random coordinates), a third deletes of stored entries."""
    nnz = len(col)
    rows = np.searchsorted(rp, rng.integers(0, nnz, k), side="right") - 1
    recs = []
    for t in range(k):
        p = int(rng.integers(rp[rows[t]], rp[rows[t] + 1])) if rp[rows[t] + 1] > rp[rows[t]] else None
        if t % 3 == 1 or p is None:
            recs.append((int(rng.integers(n)), int(rng.integers(n)), 1.5))
        else:
            recs.append((int(rows[t]), int(col[p]), 2.5 if t % 3 == 0 else None))
    return recs


def apply_edits(A, recs):
    for i, j, x in recs:
        if x is None:
            del A[i, j]
        else:
            A[i, j] = x


def routes(gb, args, rec, make, call):
    for route in ("1", "0"):
        os.environ["GRB_MI355X_EDIT"] = route
        wall, event = measure(gb, args.reps, make, call)
        rec["device" if route == "1" else "host_route"] = {"wall_ms": wall, "event_ms": event, "plan": gb.last_kernel_plan()[:80]}
    os.environ.pop("GRB_MI355X_EDIT", None)
    emit(args.out, rec)


def big(args):
    import pygraphblas_amd as gb
    from pygraphblas_amd import rmat
    rng = np.random.default_rng(7)
    for scale in args.scales:
        n = 1 << scale
        rp, col = rmat.csr_numpy(scale, seed=42)
        nnz = len(col)
        A0 = gb.Matrix.from_csr(gb.FP64, n, n, rp, col, np.ones(nnz, np.float64))          # HBM only
        u = gb.Vector.dense(gb.FP64, n, fill=1.0)
        absent = next((i, j) for i, j in ((int(rng.integers(n)), int(rng.integers(n))) for _ in range(100)) if j not in col[rp[i]:rp[i + 1]])
        recs = mixed_edits(rng, rp.astype(np.int64), col, n, 4096)

        def pair(A):
            A[absent] = 3.0
            A.mxv(u, semiring=gb.FP64.PLUS_TIMES)

        def triple(A):
            apply_edits(A, recs)
            A.nvals
            A.mxv(u, semiring=gb.FP64.PLUS_TIMES)

        def queue_edits(A):
            apply_edits(A, recs)

        def flush_only(A):
            A.nvals

        def resize(A):
            gb.lib.GrB_Matrix_resize(A._h, C.c_uint64(n), C.c_uint64(n // 2))
            A.nvals

        base = {"probe": "big", "scale": scale, "matrix_entries": int(nnz)}
        routes(gb, args, dict(base, call="pair: one insert + mxv"), A0.dup, pair)
        routes(gb, args, dict(base, call="triple: 4096 mixed edits + flush + mxv"), A0.dup, triple)
        routes(gb, args, dict(base, call="resize to half the columns"), A0.dup, resize)
        # the flush by itself (device route): the 4 096 records are queued BEFORE the interval opens, which then holds the whole flush — the upload of the list,
        # k_edit_locate, the read-back of the class bytes, the row pointer, the stream pass and the placing.  The rate is the CSR arrays the stream pass reads and
        # writes over that whole time: a lower bound of the pass's own rate.  The resize likewise: k_keep_cols_below + csr_compact (flags, scan, gather, its read-back).
        os.environ.pop("GRB_MI355X_EDIT", None)
        wall, event = measure(gb, args.reps, A0.dup, flush_only, prepare=queue_edits)
        emit(args.out, dict(base, call="whole structural flush of 4096 queued edits", event_ms=event, wall_ms=wall, GBps_csr_arrays_over_the_whole_flush=round(2 * nnz * 12 / (event * 1e-3) / 1e9, 1)))
        kept = int(np.count_nonzero(col < n // 2))
        wall, event = measure(gb, args.reps, A0.dup, resize)
        emit(args.out, dict(base, call="resize to half the columns: keep bytes + csr_compact", event_ms=event, wall_ms=wall, kept_entries=kept,
                            GBps_arrays_over_the_whole_call=round((nnz * 13 + kept * 12) / (event * 1e-3) / 1e9, 1)))
        del A0, u


def sweep(args):
    import pygraphblas_amd as gb
    rng = np.random.default_rng(9)
    for entries in (10 ** 3, 10 ** 4, 10 ** 5, 10 ** 6, 10 ** 7):
        n = max(64, entries // 16)
        keys = np.unique(rng.integers(0, n * n, entries))
        rows, col = np.divmod(keys, n)
        rp = np.zeros(n + 1, np.int64); np.add.at(rp, rows + 1, 1); rp = np.cumsum(rp)
        A0 = gb.Matrix.from_csr(gb.FP64, n, n, rp.astype(np.uint32), col.astype(np.uint32), np.ones(len(col), np.float64))
        u = gb.Vector.dense(gb.FP64, n, fill=1.0)
        for k in (1, 64, 4096):
            recs = mixed_edits(rng, rp, col, n, k)

            def call(A):
                apply_edits(A, recs)
                A.mxv(u, semiring=gb.FP64.PLUS_TIMES)              # the next kernel: on the host route it pays the rebuild and the upload

            routes(gb, args, {"probe": "sweep", "matrix_entries": int(len(col)), "edits": k, "call": "edits + the next mxv"}, A0.dup, call)
        del A0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="big")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scales", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_probe.jsonl"))
    args = ap.parse_args()
    import pygraphblas_amd as gb
    if not gb.device_info()["ok"]:
        sys.exit("edit_probe.py measures on the GPU: no HIP device")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    {"big": big, "sweep": sweep}[args.what](args)
