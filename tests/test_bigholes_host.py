"""The constants of the "big holes" product of GrB_mxv / GrB_vxm (grb_bigholes.hpp: the fill, the threshold and the four limits on |A| and |u| that keep a
MIN_PLUS / MAX_PLUS sweep over an operand with holes exact) against wide-integer and floating-point arithmetic: a stand-alone host program,
tests/bigholes_check.cpp, built plainly and under the address and undefined-behaviour sanitizers.  No device, nothing loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "bigholes_check.cpp")
INC = "-I" + os.path.join(ROOT, "pygraphblas_amd", "csrc")


def run_check(cmd, exe):
    subprocess.check_call(cmd)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "big holes ok" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]


def test_big_holes_constants(tmp_path):
    """Host compiler, no HIP: the header is plain C++."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "bigholes_check")
    run_check([cxx, "-std=c++20", "-O1", INC, SRC, "-o", exe], exe)


def test_big_holes_constants_under_the_sanitizers(tmp_path):
    """The same program as the device compiler's host pass sees the header, with the address and undefined-behaviour sanitizers: a host program of its own, no
    device code."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "bigholes_check_san")
    run_check([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++20", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
               INC, SRC, "-o", exe], exe)
