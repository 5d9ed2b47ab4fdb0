#!/usr/bin/env python3
"""Writes tests/golden/tile_pipeline_digests.json from the library that is loaded (GRB_MI355X_LIB selects a build of another
commit): run it on the commit whose bits tests/test_tile_pipeline_bits_gpu.py is to hold later ones to.  Needs the GPU.
  python tests/golden/make_tile_pipeline_digests.py [out.json]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import torch
import pygraphblas_amd as gb
import test_tile_pipeline_bits_gpu as T

out = {}
for case in T.CASES:
    out[case], plan = T.digests(gb, torch, torch.device("cuda", 0), case)
    assert "k_spmv_xcd" in plan, plan
    out[case]["plan"] = plan.strip()
    print(case, out[case], flush=True)
json.dump(out, open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "tile_pipeline_digests.json"), "w"), indent=1)
