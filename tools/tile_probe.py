#!/usr/bin/env python3
"""Measurement harness: GxB_Matrix_concat / GxB_Matrix_split, device route (grb_tile.hip) against the host route of grb_tile_ops.cpp (GRB_MI355X_TILE=0), same
binary, fresh inputs per call, one process.

  --what sweep   the two dispatch thresholds: FP64 operands of 1e2 .. 1e7 entries whose only valid image is the HOST mirror (about eight entries per row), a
                 2 x 2 grid; one call on each route, upload included, the median of --reps calls after a warm-up.  The threshold of an entry point is the
                 smallest decade from which the device route wins and keeps winning.
  --what big     R-MAT matrices (--scales, default 20 22) FP64 that live in HBM only, split 8 x 8 and concatenated back, whole-call HIP-event time, the mean of
                 --reps calls after a warm-up, beside (a) a device-to-device copy of the same bytes (rowptr + col + val, read once and written once), (b) the
                 existing way: 64 ranged extract_matrix calls / 64 ranged assign_matrix calls into a prepared C, and (c) for 1 x 2, dist.split_csr_columns.
Every step runs under --step-seconds (SIGALRM) and the probe stops at the first failure.  One JSON line per measurement is appended to --out (default
profiles/tile_probe.jsonl).  Run each --what as its own command under `timeout`."""
import argparse
import ctypes as C
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def emit(out, rec):
    print(json.dumps(rec), flush=True)
    with open(out, "a") as f:
        f.write(json.dumps(rec) + "\n")


class step:
    """A time limit for one step: the probe ends there (nothing more is started on the GPU)."""
    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def __enter__(self):
        def over(signum, frame):
            sys.exit(f"tile_probe.py: step '{self.what}' passed its limit of {self.seconds} s")
        signal.signal(signal.SIGALRM, over)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def halves(n):
    return [n // 2, n - n // 2]


def timed_routes(gb, rec, reps, make, call, plan_prefix):
    for route in ("1", "0"):
        os.environ["GRB_MI355X_TILE"] = route
        walls = []
        for rep in range(reps + 1):                                 # the first repetition is the warm-up
            operand = make()                                        # host mirrors only: the device route uploads inside the call
            gb.lib.GrBX_device_synchronize()
            t0 = time.perf_counter()
            result = call(operand)
            gb.lib.GrBX_device_synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
            assert gb.last_kernel_plan().startswith(plan_prefix) == (route == "1"), gb.last_kernel_plan()
            del operand, result
        rec["device_wall_ms_with_upload" if route == "1" else "host_wall_ms"] = round(float(np.median(walls[1:])), 4)
    rec["device_wins"] = rec["device_wall_ms_with_upload"] < rec["host_wall_ms"]
    os.environ.pop("GRB_MI355X_TILE", None)


def sweep(args):
    import pygraphblas_amd as gb
    for entries in (100, 1000, 10000, 100000, 1000000, 10000000):
        rng = np.random.default_rng(3 + entries)
        n = max(entries // 8, 4)
        keys = np.unique(rng.integers(0, n * n, entries, dtype=np.int64))
        I, J = np.divmod(keys, n)
        X = rng.random(len(keys))
        rows, cols = halves(n), halves(n)
        with step(args.step_seconds, f"split {entries}"):
            rec = {"probe": "sweep", "entry_point": "GxB_Matrix_split", "operand_entries": int(len(keys)), "n": int(n), "grid": "2x2"}
            timed_routes(gb, rec, args.reps, lambda: gb.Matrix.from_arrays(I.astype(np.uint64), J.astype(np.uint64), X, n, n, gb.FP64), lambda A: A.split(rows, cols), "split<")
            emit(args.out, rec)
        tiles = []
        for a in range(2):
            for b in range(2):
                keep = ((I >= a * rows[0]) & (I < (rows[0] if a == 0 else n))) & ((J >= b * cols[0]) & (J < (cols[0] if b == 0 else n)))
                tiles.append(((I[keep] - a * rows[0]).astype(np.uint64), (J[keep] - b * cols[0]).astype(np.uint64), X[keep], rows[a], cols[b]))
        with step(args.step_seconds, f"concat {entries}"):
            rec = {"probe": "sweep", "entry_point": "GxB_Matrix_concat", "operand_entries": int(len(keys)), "n": int(n), "grid": "2x2"}
            make = lambda: [[gb.Matrix.from_arrays(*tiles[a * 2 + b][:3], tiles[a * 2 + b][3], tiles[a * 2 + b][4], gb.FP64) for b in range(2)] for a in range(2)]
            timed_routes(gb, rec, args.reps, make, lambda g: gb.Matrix.concat(g), "concat<")
            emit(args.out, rec)


def event_ms(gb, reps, call):
    times, out = [], None
    for rep in range(reps + 1):                                     # the first repetition is the warm-up (code object, pool)
        del out
        gb.lib.GrBX_device_synchronize()
        gb.lib.GrBX_timer_start()
        out = call()
        ms = C.c_float(0); gb.lib.GrBX_timer_stop(C.byref(ms))
        times.append(ms.value)
    return round(float(np.mean(times[1:])), 4), out


def big(args):
    import torch
    import pygraphblas_amd as gb
    from pygraphblas_amd import rmat, dist
    os.environ.pop("GRB_MI355X_TILE", None)                         # default routing: HBM-only operands take the device route by themselves
    for scale in args.scales:
        n = 1 << scale
        rp, col = rmat.csr_numpy(scale, seed=42)
        nnz = int(len(col))
        A = gb.Matrix.from_csr(gb.FP64, n, n, rp.astype(np.uint32), col.astype(np.uint32), np.ones(nnz))      # HBM only
        sizes = [n // 8] * 8
        bytes_moved = 2 * (4 * (n + 1) + 12 * nnz)                  # rowptr + col + val, read once and written once
        rec = {"probe": "big", "scale": scale, "entries": nnz, "grid": "8x8", "bytes_read_and_written": bytes_moved}
        with step(args.step_seconds, f"split 8x8 scale {scale}"):
            rec["split_event_ms"], parts = event_ms(gb, args.reps, lambda: A.split(sizes, sizes))
            assert gb.last_kernel_plan().startswith("split<")
        with step(args.step_seconds, f"concat 8x8 scale {scale}"):
            rec["concat_event_ms"], back = event_ms(gb, args.reps, lambda: gb.Matrix.concat(parts))
            assert gb.last_kernel_plan().startswith("concat<") and back.nvals == nnz
        with step(args.step_seconds, f"copy scale {scale}"):
            src = torch.empty(bytes_moved // 2, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
            torch.cuda.synchronize()
            times = []
            for rep in range(args.reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); dst.copy_(src); e1.record(); torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
            rec["copy_event_ms"] = round(float(np.mean(times[1:])), 4)
            rec["split_fraction_of_copy_rate"] = round(rec["copy_event_ms"] / rec["split_event_ms"], 4)
            rec["concat_fraction_of_copy_rate"] = round(rec["copy_event_ms"] / rec["concat_event_ms"], 4)
            del src, dst
        b = np.arange(0, n + 1, n // 8)
        with step(args.step_seconds, f"64 extracts scale {scale}"):
            rec["extract_64_calls_event_ms"], _ = event_ms(gb, 1, lambda: [A.extract_matrix(slice(int(b[x]), int(b[x + 1]) - 1), slice(int(b[y]), int(b[y + 1]) - 1)) for x in range(8) for y in range(8)])
        with step(args.step_seconds, f"64 assigns scale {scale}"):
            def assign_all():
                out = gb.Matrix.sparse(gb.FP64, n, n)
                for x in range(8):
                    for y in range(8):
                        out.assign_matrix(parts[x][y], slice(int(b[x]), int(b[x + 1]) - 1), slice(int(b[y]), int(b[y + 1]) - 1))
                return out
            rec["assign_64_calls_event_ms"], _ = event_ms(gb, 1, assign_all)
        with step(args.step_seconds, f"1x2 scale {scale}"):
            rec["split_1x2_event_ms"], _ = event_ms(gb, args.reps, lambda: A.split([n], [n // 2, n - n // 2]))
            trp, tcol, tval = A.to_csr_tensors()
            rec["dist_split_csr_columns_event_ms"], _ = event_ms(gb, args.reps, lambda: (dist.split_csr_columns(trp, tcol, 0, n // 2, tval), torch.cuda.synchronize()))
        emit(args.out, rec)
        del A, parts, back


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="sweep")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scales", type=int, nargs="+", default=[20, 22])
    ap.add_argument("--step-seconds", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_probe.jsonl"))
    args = ap.parse_args()
    import pygraphblas_amd as gb
    if not gb.device_info()["ok"]:
        sys.exit("tile_probe.py measures on the GPU: no HIP device")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    {"sweep": sweep, "big": big}[args.what](args)
