"""The transitions of grb_devcsr.hpp (what the library derives from a matrix's device CSR, and the only code that clears it) on a CSR with every derived field
set and every buffer allocated: a stand-alone host program, tests/csr_derived_check.cpp, built plainly and under the address and undefined-behaviour sanitizers.
No device, nothing loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csr_derived_check.cpp")
INC = "-I" + os.path.join(ROOT, "pygraphblas_amd", "csrc")


def run_check(cmd, exe):
    subprocess.check_call(cmd)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "csr derived ok" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]


def test_csr_derived_transitions(tmp_path):
    """Host compiler, no HIP: the header is plain C++ and only declares the allocator."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "csr_derived_check")
    run_check([cxx, "-std=c++20", "-O1", INC, SRC, "-o", exe], exe)


def test_csr_derived_transitions_under_the_sanitizers(tmp_path):
    """The same program as the device compiler's host pass sees the header, with the address and undefined-behaviour sanitizers: a host program of its own."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "csr_derived_check_san")
    run_check([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++20", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
               INC, SRC, "-o", exe], exe)
