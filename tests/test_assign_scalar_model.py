"""The parts of the matrix scalar assign that need no device: the two formulations of its model (tests/assign_scalar_model.py) agree — T as the full block and
T restricted to the mask's true entries, which is what lets the device route build T from the mask's pattern —, the model gives the results the reference's
docstrings print (tests/golden/reference_assign_scalar_docs.json), and the region arithmetic of grb_assign_scalar_geom.hpp passes its stand-alone check under
the address and undefined-behaviour sanitizers (tests/assign_scalar_geometry_check.cpp: a host program of its own, nothing loaded into Python)."""
import json
import os
import shutil
import subprocess

import numpy as np

import assign_scalar_model as model
import matrix_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = ["BOOL", "INT8", "UINT8", "INT16", "UINT16", "INT32", "UINT32", "INT64", "UINT64", "FP32", "FP64"]


def random_mat(rng, nrows, ncols, typ, density):
    total = nrows * ncols
    keys = np.sort(rng.choice(total, size=int(round(total * density)), replace=False)).astype(np.int64)
    vals = rng.integers(0, 2 if typ == "BOOL" else 4, len(keys)).astype(mm.NP[typ])      # explicit zeros included
    return mm.Mat(nrows, ncols, keys, vals)


def random_indices(rng, d):
    kind = rng.integers(0, 5)
    if kind == 0:
        return list(range(d))
    if kind == 1:
        return []
    if kind == 2:
        return [int(rng.integers(0, d))]
    k = int(rng.integers(1, d + 1))
    return [int(x) for x in rng.permutation(d)[:k]]


def same(a, b):
    return a.typ == b.typ and np.array_equal(a.keys, b.keys) and np.array_equal(a.vals, b.vals)


def test_the_block_and_the_masks_true_entries_give_the_same_result():
    """C<M>(I, J) = accum(C(I, J), s) reads T only where M allows a write: T = the full block and T = M's true entries inside I x J are the same operation, for
    valued and structural masks, with and without replace and an accumulator, M of another type than C, M empty, M the same matrix as C."""
    rng = np.random.default_rng(20240)
    ran = 0
    for i in range(400):
        nr, nc = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        ctyp, mtyp = TYPES[i % 11], TYPES[(i * 5 + 2) % 11]
        C = random_mat(rng, nr, nc, ctyp, float(rng.choice([0.0, 0.3, 0.8])))
        M = C if i % 13 == 0 else random_mat(rng, nr, nc, mtyp, float(rng.choice([0.0, 0.2, 0.6, 1.0])))
        rows, cols = random_indices(rng, nr), random_indices(rng, nc)
        struct, replace = bool((i // 2) % 2), bool((i // 4) % 2)
        accum = [None, ("PLUS", ctyp), ("MIN", ctyp), ("TIMES", ctyp), ("PLUS", "INT32")][(i // 3) % 5]
        s = int(rng.integers(0, 4))
        full = model.assign_scalar(C, s, rows, cols, M, struct, False, replace, accum)
        part = model.assign_scalar_restricted(C, s, rows, cols, M, struct, replace, accum)
        assert same(full, part), (i, ctyp, mtyp, rows, cols, struct, replace, accum)
        ran += 1
    assert ran == 400


def test_the_model_on_hand_worked_cases():
    """The rule itself, on cases small enough to state: entries outside the region stay, entries inside are replaced or accumulated, a complemented mask keeps
    the masked positions, replace deletes what the mask does not allow — anywhere in C."""
    C = mm.from_coo(3, 3, [0, 1, 2], [0, 1, 2], [5, 6, 7], "INT32")
    out = model.assign_scalar(C, 9, [1], [0, 1])
    assert out.keys.tolist() == [0, 3, 4, 8] and out.vals.tolist() == [5, 9, 9, 7]
    out = model.assign_scalar(C, 9, [1], [0, 1], accum=("PLUS", "INT32"))
    assert out.keys.tolist() == [0, 3, 4, 8] and out.vals.tolist() == [5, 9, 15, 7]
    M = mm.from_coo(3, 3, [1, 1, 2], [0, 1, 2], [1, 0, 1], "UINT8")
    out = model.assign_scalar(C, 9, [0, 1, 2], [0, 1, 2], M)                  # (1,1) holds an explicit zero: not allowed; (2,2) is
    assert out.keys.tolist() == [0, 3, 4, 8] and out.vals.tolist() == [5, 9, 6, 9]
    out = model.assign_scalar(C, 9, [1], [0, 1, 2], M, replace=True)           # replace spans all of C: (0,0) and (1,1) go; (2,2) is allowed and outside the region: kept
    assert out.keys.tolist() == [3, 8] and out.vals.tolist() == [9, 7]
    out = model.assign_scalar(C, 9, [1], [0, 1, 2], M, comp=True)
    assert out.keys.tolist() == [0, 4, 5, 8] and out.vals.tolist() == [5, 9, 9, 7]
    out = model.assign_scalar(C, 9, [1], [0, 1, 2], M, struct=True)
    assert out.keys.tolist() == [0, 3, 4, 8] and out.vals.tolist() == [5, 9, 9, 7]


def test_the_model_gives_the_references_docstring_results():
    with open(os.path.join(ROOT, "tests", "golden", "reference_assign_scalar_docs.json")) as f:
        doc = json.load(f)
    nr, nc = doc["nrows"], doc["ncols"]

    def positions(x, d):
        return list(range(d)) if x is None else ([x] if isinstance(x, int) else x)
    for case in doc["cases"]:
        out = model.assign_scalar(mm.empty(nr, nc, doc["type"]), doc["value"], positions(case["rows"], nr), positions(case["cols"], nc))
        assert [[int(k) // nc, int(k) % nc] for k in out.keys] == case["entries"] and out.vals.all(), case["form"]
    for case in doc["sparse_fill"]:
        i, j = case["mask_entry"]
        M = mm.from_coo(4, 4, [i], [j], [True], "BOOL")
        out = model.assign_scalar_restricted(mm.empty(4, 4, case["type"]), 0.0 if case["fill"] is None else case["fill"], range(4), range(4), M)
        assert [[int(k) // 4, int(k) % 4, float(v)] for k, v in zip(out.keys, out.vals)] == case["tuples"]


def test_region_geometry_under_the_sanitizers(tmp_path):
    """The size test of I x J at 65 535^2, 65 536^2, 0xFFFFFFF0 and 0xFFFFFFF1 against 128-bit arithmetic, range triples (step 0, both directions) and the block's
    column slots against enumeration: a host program of its own, host code only, built with the address and undefined-behaviour sanitizers."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "assign_scalar_geometry_check")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++20", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "pygraphblas_amd", "csrc"), os.path.join(ROOT, "tests", "assign_scalar_geometry_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "assign scalar geometry ok" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
