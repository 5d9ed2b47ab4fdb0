"""Kernel X's tile pipeline (pygraphblas_amd/csrc/grb_spmv_tiles.hpp) must give the SAME BITS as the commit before its
vector-memory diet (tile metadata through the scalar cache, table fill behind the first column loads): tiles, scan order and merge
are unchanged, so the association of every sum is, and `w` may not differ in one bit.

tests/golden/tile_pipeline_digests.json holds SHA-256 digests taken on that parent commit (tests/golden/make_tile_pipeline_digests.py):
  fp64_plus_times   what `bench.py --dump-outputs DIR` writes at its default arguments (R-MAT-22, seeds 42 / 43 / 44): the digest of
                    DIR/w_indices.npy and DIR/w_values.npy, recomputed here in-process
  fp32_plus_second  the pattern product of PageRank: the 32-bit entry-word format of the pipeline
  int64_min_plus    weights 1 ... 255 in INT64: the 16-bit column plane with the narrow (int16) value plane
each as the digest of the .npy image (float64, as bench.py dumps) of w's indices and values.
"""
import hashlib
import io
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCALE = 22
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tile_pipeline_digests.json")
CASES = ["fp64_plus_times", "fp32_plus_second", "int64_min_plus"]


def npy_sha256(a):
    """SHA-256 of the file `np.save` writes for `a` as float64 (bench.py's dump format)."""
    buf = io.BytesIO()
    np.save(buf, np.asarray(a).astype(np.float64))
    return hashlib.sha256(buf.getvalue()).hexdigest()


def product(gb, torch, dev, case):
    """(w's indices, w's values, the plan string of the last product) of the case's product, run until kernel X's plan is the one running."""
    from pygraphblas_amd import rmat
    n = 1 << SCALE
    if case == "fp64_plus_times":              # bench.py's SpmvJob
        rowptr, col = rmat.csr_torch(SCALE, dev, seed=42)
        nnz = int(col.numel())
        vals = rmat.values_torch(nnz, dev, seed=43)
        xs = rmat.values_torch(n, dev, seed=44)
        typ, sr = gb.FP64, gb.FP64.PLUS_TIMES
    elif case == "fp32_plus_second":
        rowptr, col = rmat.csr_torch(SCALE, dev, seed=42)
        nnz = int(col.numel())
        vals = torch.ones(nnz, dtype=torch.float32, device=dev)
        xs = rmat.values_torch(n, dev, seed=44, dtype=torch.float32)
        typ, sr = gb.FP32, gb.FP32.PLUS_SECOND
    else:                                      # bench.py's SSSP weights
        rowptr, col = rmat.csr_torch(SCALE, dev, seed=42, drop_self_loops=True)
        nnz = int(col.numel())
        vals = (rmat.values_torch(nnz, dev, seed=47) * 255.0).to(torch.int64) + 1
        xs = (rmat.values_torch(n, dev, seed=44) * 1000.0).to(torch.int64)
        typ, sr = gb.INT64, gb.INT64.MIN_PLUS
    A = gb.Matrix.from_csr(typ, n, n, rowptr.data_ptr(), col.data_ptr(), (vals.data_ptr(), nnz), device=True)
    x = gb.Vector.from_dense_array((xs.data_ptr(), n), typ, device=True)
    w = gb.Vector.sparse(typ, n)
    for _ in range(3):                         # two warm-up products (kernel W, then kernel X's plan is built), then the one compared
        A.mxv(x, semiring=sr, out=w)
    plan = gb.last_kernel_plan()
    I, X = w.to_arrays()
    return I, X, plan


def digests(gb, torch, dev, case):
    I, X, plan = product(gb, torch, dev, case)
    return {"w_indices_sha256": npy_sha256(I), "w_values_sha256": npy_sha256(X), "nvals": int(len(I))}, plan


@pytest.mark.parametrize("case", CASES)
def test_tile_pipeline_gives_the_parent_commits_bits(gb, gpu, case):
    import torch
    want = json.load(open(GOLDEN))[case]
    got, plan = digests(gb, torch, torch.device("cuda", 0), case)
    assert "k_spmv_xcd" in plan, plan
    assert ("values=int16" in plan) == (case == "int64_min_plus"), plan
    print(case, plan.strip(), got)
    assert got["nvals"] == want["nvals"]
    assert got["w_indices_sha256"] == want["w_indices_sha256"]
    assert got["w_values_sha256"] == want["w_values_sha256"], "the sums' association changed: w differs from the parent commit's in some bit"
