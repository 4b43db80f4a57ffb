"""The launch plan of the 16-bit forward (mapf_gpt_amd/csrc/gpt_plan.h) is host logic: checked here without a device."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_plan_table_grid_and_invariants(tmp_path):
    """tests/host/plan_check.cpp: every cell of the table of DESIGN.md section 3.2 by hand-written expectation, every Plan field over
    the grid of tests/host/plan_expected.txt (4080 cases, the output of the make_plan that read ModeState's flags and pointers), and
    the plan's invariants over the same grid; built with AddressSanitizer + UBSan as a program of its own and run directly."""
    from mapf_gpt_amd import build
    # the compiler behind hipcc first: clang links the sanitizer runtime statically, so the program does not care what else is loaded
    rocm_clang = os.path.join(os.path.dirname(os.path.realpath(build.HIPCC)), "..", "lib", "llvm", "bin", "clang++")
    cxx = next((c for c in (os.environ.get("CXX"), rocm_clang, "clang++", "c++", "g++") if c and shutil.which(c)), None)
    assert cxx is not None, "no C++ compiler found"
    exe = str(tmp_path / "plan_check")
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "plan_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "host", "plan_expected.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plan_check: ok (72 cells, 4080 grid cases)" in r.stdout and "Sanitizer" not in r.stderr, r.stdout + r.stderr
