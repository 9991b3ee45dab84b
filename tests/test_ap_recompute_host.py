"""csrc/skew_geometry.hpp and LoopShape::ap_recomputed (csrc/slab_decisions.hpp): the skewed block tiles of the r update that recomputes
A p', the eligibility rule on the fused launch's block map and the decision itself need no HIP. tests/abi/skew_geometry_test.cpp
includes those two headers and standard headers only, is compiled with g++ -fsanitize=address,undefined and run as it is, a program
of its own."""
import os
import subprocess

from conftest import ROOT


def test_skew_geometry_and_decision_under_sanitizers(tmp_path):
    exe = tmp_path / "skew_geometry_test"
    build = subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
                            "-I", os.path.join(ROOT, "cuda-spmv-benchmark_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "skew_geometry_test.cpp"),
                            "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "skew_geometry: ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
