"""csrc/slab_decisions.hpp, LoopShape::first_recomputed / first_form and default_block_rows: whether iteration 0 leaves A p0 unstored,
which vector its r update then reads, and how many grid rows a block tile gets by default need no HIP.
tests/abi/first_recompute_test.cpp includes that header and standard headers only, is compiled with
g++ -fsanitize=address,undefined and run as it is, a program of its own."""
import os
import subprocess

from conftest import ROOT


def test_first_recompute_decisions_under_sanitizers(tmp_path):
    exe = tmp_path / "first_recompute_test"
    build = subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
                            "-I", os.path.join(ROOT, "cuda-spmv-benchmark_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "first_recompute_test.cpp"),
                            "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "first_recompute: ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
