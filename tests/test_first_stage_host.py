"""csrc/slab_decisions.hpp, LoopShape::b_is_p0 and sums_to_plus_zero: the decision that b serves as p0 and the matrix fact it rests on
need no HIP. tests/abi/slab_first_stage_test.cpp includes that header and standard headers only, is compiled with
g++ -fsanitize=address,undefined and run as it is, a program of its own."""
import os
import subprocess

from conftest import ROOT


def test_first_stage_decision_under_sanitizers(tmp_path):
    exe = tmp_path / "slab_first_stage_test"
    build = subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
                            "-I", os.path.join(ROOT, "cuda-spmv-benchmark_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "slab_first_stage_test.cpp"),
                            "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "slab_first_stage: ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
