"""CPU checks of bf16 mixed-precision training: the training CLI's --dtype (train.py:66-70), the binding of mgpt_gpt_forward_backward_prec, and
that the bf16 training kernels (mapf_gpt_amd/csrc/gpt_kernels_train_bf16.h) compile for gfx950 without scratch."""
import ctypes
import os
import re
import subprocess

import pytest

from mapf_gpt_amd import _lib, training
from tests.helpers import ROOT

REQUIRED = ["--init", "tiny", "--data", "a.arrow", "--val", "b.arrow"]


def test_dtype_flag():
    assert training.parse_args(REQUIRED).precision == "f32"                       # the default stays exact fp32
    a = training.parse_args(REQUIRED + ["--dtype", "bfloat16"])
    assert (a.dtype, a.precision) == ("bfloat16", "bf16")
    assert training.parse_args(REQUIRED + ["--dtype", "float32"]).precision == "f32"
    assert training.DTYPES == {"float32": "f32", "bfloat16": "bf16"}
    assert "train.py itself defaults to bfloat16" in " ".join(training.__doc__.split())


def test_dtype_float16_is_refused(capfd):
    with pytest.raises(SystemExit) as e:
        training.parse_args(REQUIRED + ["--dtype", "float16"])
    assert e.value.code == 2
    assert "GradScaler" in capfd.readouterr().err
    with pytest.raises(SystemExit):
        training.parse_args(REQUIRED + ["--dtype", "int8"])


def test_forward_backward_prec_binding():
    src = open(os.path.join(ROOT, "include", "mapf_gpt_amd.h")).read()
    decl = re.search(r"int mgpt_gpt_forward_backward_prec\((.*?)\);", src, flags=re.S)
    assert decl is not None
    assert len(decl.group(1).split(",")) == 9 and "int precision" in decl.group(1)
    res, args = _lib.SYMBOLS["mgpt_gpt_forward_backward_prec"]
    assert res is ctypes.c_int and len(args) == 9 and args[7] is ctypes.c_int


def test_forward_backward_prec_argument_checks_without_gpu():
    from mapf_gpt_amd import build
    build.build()
    L = _lib.lib()
    assert L.mgpt_gpt_forward_backward_prec(None, None, 1, 256, None, 1.0, None, _lib.PREC_BF16, None) == _lib.ERR_ARG
    assert b"NULL" in L.mgpt_last_error()


def test_bf16_training_kernels_use_no_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    csrc = os.path.join(ROOT, "mapf_gpt_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(csrc, "train.hip"), "-o", str(tmp_path / "train.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            kernels[cur] = int(m.group(1))
    new = {k: v for k, v in kernels.items() if "3tbk" in k}
    assert len(new) >= 12, sorted(kernels)
    assert all(v == 0 for v in new.values()), new
