"""CPU-side checks of the C-ABI library: it loads, exports every symbol the header declares, and
refuses to compute without a device (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from mapf_gpt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from mapf_gpt_amd import build
    build.build()
    return _lib.lib()


def header_symbols():
    src = open(os.path.join(ROOT, "include", "mapf_gpt_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mgpt_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol(L):
    syms = header_symbols()
    assert len(syms) >= 25
    for s in syms:
        assert hasattr(L, s), f"{s} declared in include/mapf_gpt_amd.h but not exported"
    assert set(syms) == set(_lib.SYMBOLS), set(syms) ^ set(_lib.SYMBOLS)


def test_version_and_error_string(L):
    assert L.mgpt_abi_version() == 1003
    rc = L.mgpt_gpt_create(None, 1, 1, 32, 256, 1)
    assert rc == _lib.ERR_ARG and b"NULL" in L.mgpt_last_error()


def test_argument_validation_without_gpu(L):
    h = ctypes.c_void_p()
    assert L.mgpt_gpt_create(ctypes.byref(h), 2, 2, 64, 257, 4) == _lib.ERR_UNSUPPORTED      # block_size 1 .. 256
    assert L.mgpt_gpt_create(ctypes.byref(h), 2, 2, 64, 0, 4) == _lib.ERR_UNSUPPORTED
    assert L.mgpt_gpt_create(ctypes.byref(h), 2, 3, 64, 256, 4) == _lib.ERR_ARG              # n_embd % n_head
    # InputParameters (observation_generator.h:22-40): non-default values are honoured inside the kernels' layout bounds
    # (tests/test_gpu_tokenizer.py::test_non_default_input_parameters_vs_reference_goldens); outside them the call refuses
    for bad in [(20, 17, 5, 256, 5, 5),      # more than 16 record slots
                (20, 13, 6, 256, 5, 5),      # more than five previous actions (AgentRec::hist)
                (20, 13, 5, 256, 6, 5),      # obs radius 6: 169 window cells
                (20, 13, 5, 256, 5, 6),      # agents radius 6
                (3, 13, 5, 256, 5, 5),       # agents radius above the value limit: the reference throws (cpp:358-359)
                (20, 16, 5, 256, 5, 5),      # 121 + 16 * 10 tokens do not fit a 256-token row
                (20, 13, 5, 128, 5, 5),      # rows are 256 tokens whatever context_size says (cpp:386)
                (0, 13, 5, 256, 5, 5)]:
        st = _lib.InputParametersStruct(*bad, 64, 0)
        assert L.mgpt_tokenizer_create(ctypes.byref(h), ctypes.byref(st), 1, 4, 20, 20, 1) == _lib.ERR_UNSUPPORTED, bad


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a box without a GPU")
def test_no_cpu_fallback():
    from mapf_gpt_amd.observation_generator import BatchedTokenizer
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BatchedTokenizer(np.zeros((20, 20), np.uint8), 1, 2)
    from mapf_gpt_amd.inference import MAPFGPTInference, MAPFGPTInferenceConfig
    with pytest.raises(RuntimeError):
        MAPFGPTInference(MAPFGPTInferenceConfig(path_to_weights="synthetic:tiny"))


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a box without a GPU")
def test_failed_create_leaves_nothing_behind(L):
    """Without a device every create with valid arguments fails at its first allocation: ERR_HIP, a NULL handle, and nothing
    left in the arenas (mgpt_mem_debug)."""
    assert _lib.mem_debug() == (0, 0)
    cfg = _lib.InputParametersStruct(20, 13, 5, 256, 5, 5, 64, 0)
    grid = np.zeros((20, 20), np.uint8)
    creates = {
        "env": lambda h: L.mgpt_env_create(ctypes.byref(h), 2, 4, 20, 20, 1, 16),
        "tokenizer": lambda h: L.mgpt_tokenizer_create(ctypes.byref(h), ctypes.byref(cfg), 2, 4, 20, 20, 1),
        "gpt": lambda h: L.mgpt_gpt_create(ctypes.byref(h), 2, 2, 64, 256, 2),
        "dedup": lambda h: L.mgpt_dedup_create(ctypes.byref(h), 64, 64, None),
        "dataset": lambda h: L.mgpt_dataset_create(ctypes.byref(h), ctypes.c_void_p(grid.ctypes.data), 20, 20, None),
    }
    for name, create in creates.items():
        h = ctypes.c_void_p()
        assert create(h) == _lib.ERR_HIP, (name, L.mgpt_last_error())
        assert not h, name
        assert _lib.mem_debug() == (0, 0), name


def test_arena_bookkeeping_under_sanitizers(tmp_path):
    """tests/host/arena_check.cpp: mgpt::Arena on malloc / free (alloc, release, move, adopt, reuse, a failure at every step of a
    five-allocation sequence), built with AddressSanitizer + UBSan as a program of its own and run directly."""
    import shutil
    import subprocess
    from mapf_gpt_amd import build
    # the compiler behind hipcc first: clang links the sanitizer runtime statically, so the program does not care what else is loaded
    rocm_clang = os.path.join(os.path.dirname(os.path.realpath(build.HIPCC)), "..", "lib", "llvm", "bin", "clang++")
    cxx = next((c for c in (os.environ.get("CXX"), rocm_clang, "clang++", "c++", "g++") if c and shutil.which(c)), None)
    assert cxx is not None, "no C++ compiler found"
    exe = str(tmp_path / "arena_check")
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "arena_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "arena_check: ok (0 allocations, 0 bytes live)" in r.stdout and "Sanitizer" not in r.stderr, r.stdout + r.stderr
