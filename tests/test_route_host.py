"""The host-or-device route policy of grb_route.hpp, without a device: the two policy functions against the nine predicates they replaced and every threshold
against its value, under the address and undefined-behaviour sanitizers (a stand-alone host program, tests/route_policy_check.cpp)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_route_policy_under_the_sanitizers(tmp_path):
    """hook x device x legality x list-in-HBM x residency x known-count x {0, min - 1, min, min + 1} for each of the ten thresholds: a host program of its own
    with the address and undefined-behaviour sanitizers; nothing is loaded into Python."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "route_policy_check")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++20", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "pygraphblas_amd", "csrc"), os.path.join(ROOT, "tests", "route_policy_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "route policy ok" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
