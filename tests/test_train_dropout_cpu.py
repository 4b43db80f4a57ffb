"""CPU checks of training dropout: the torch restatement (tests/train_dropout_ref.py) against the pinned oracle at p = 0, the statistics of
the host mask specification (mapf_gpt_amd/sampling.py: dropout_keep), the binding and GPU-free argument checks of
mgpt_gpt_forward_backward_drop, the training CLI's --dropout, and that the dropout kernel instances compile for gfx950 without scratch."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from mapf_gpt_amd import _lib, sampling, training, weights
from tests import train_dropout_ref as ref
from tests.helpers import ROOT
from tests.train_ref import loss_and_grads, trained_like_case

REQUIRED = ["--init", "tiny", "--data", "a.arrow", "--val", "b.arrow"]
N = 1 << 20


def test_restatement_at_p0_is_the_pinned_oracle():
    tokens, targets, sd, args = trained_like_case("tiny", 2)
    l0, g0 = loss_and_grads(sd, args, tokens, targets, torch.float64)
    l1, g1 = ref.loss_and_grads(sd, args, tokens, targets, 0.0, seed=3, step=5)
    assert abs(l1 - l0) <= 1e-12 * abs(l0)
    for k, v in g0.items():
        assert float((g1[k] - v).abs().max()) <= 1e-12 * float(v.abs().max()), k
    # sites = 0 is p = 0 too
    l2, _ = ref.loss_and_grads(sd, args, tokens, targets, 0.5, seed=3, step=5, sites=0)
    assert l2 == l1


def _corr_sigma(a, b):
    a, b = a - a.mean(), b - b.mean()
    return abs(float((a * b).mean() / (a.std() * b.std()))) * np.sqrt(len(a))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_mask_statistics(p):
    idx = np.arange(N)
    q = sampling.dropout_threshold(p) / 65536.0
    streams = {(site, layer, step, 0): sampling.dropout_keep(7, step, site, layer, idx, p).astype(np.float64)
               for site in range(4) for layer in (0, 1) for step in (0, 1)}
    # row0 = 1 against row0 = 0: the next row's elements (tiny: 2 heads of 65536 probabilities, 256 x 64 elements elsewhere)
    streams[(1, 0, 0, 1)] = sampling.dropout_keep(7, 0, 1, 0, idx + 2 * 65536, p).astype(np.float64)
    streams[(2, 0, 0, 1)] = sampling.dropout_keep(7, 0, 2, 0, idx + 256 * 64, p).astype(np.float64)
    sd = np.sqrt(q * (1 - q) / N)
    for k, m in streams.items():
        assert abs(m.mean() - (1 - q)) <= 5 * sd, (k, m.mean())
    for a, b in itertools.combinations(streams, 2):
        assert _corr_sigma(streams[a], streams[b]) < 5, (a, b)
    for k, m in streams.items():
        for lag in (1, 2, 3, 4, 256, 65536):
            assert _corr_sigma(m[:-lag], m[lag:]) < 5, (k, lag)


def test_every_key_component_changes_the_mask():
    idx = np.arange(4096)
    base = sampling.dropout_keep(1, 2, 1, 0, idx, 0.5)
    for args in ((2, 2, 1, 0), (1, 3, 1, 0), (1, 2, 2, 0), (1, 2, 1, 1)):
        other = sampling.dropout_keep(*args, idx, 0.5)
        assert 0.4 < (other != base).mean() < 0.6, args
    assert np.array_equal(base, sampling.dropout_keep(1, 2, 1, 0, idx, 0.5))
    # p = 0 keeps everything, the scale is the exact reciprocal of the kept share
    assert sampling.dropout_keep(1, 2, 1, 0, idx, 0.0).all() and sampling.dropout_scale(0.0) == 1.0
    assert sampling.dropout_scale(0.5) == np.float32(2.0) and sampling.dropout_threshold(0.1) == 6554
    with pytest.raises(ValueError):
        sampling.dropout_threshold(1.0)


def test_forward_backward_drop_binding_and_argument_checks():
    src = open(os.path.join(ROOT, "include", "mapf_gpt_amd.h")).read()
    decl = re.search(r"int mgpt_gpt_forward_backward_drop\((.*?)\);", src, flags=re.S)
    assert decl is not None and len(decl.group(1).split(",")) == 14
    res, args = _lib.SYMBOLS["mgpt_gpt_forward_backward_drop"]
    assert res is ctypes.c_int and len(args) == 14 and args[8] is ctypes.c_float and args[9] is ctypes.c_uint64
    from mapf_gpt_amd import build
    build.build()
    L = _lib.lib()
    for p in (1.0, -0.1, float("nan")):
        assert L.mgpt_gpt_forward_backward_drop(None, None, 1, 256, None, 1.0, None, _lib.PREC_F32, p, 0, 0, 0, 15, None) == _lib.ERR_ARG
        assert b"dropout p" in L.mgpt_last_error()
    assert L.mgpt_gpt_forward_backward_drop(None, None, 1, 256, None, 1.0, None, _lib.PREC_F32, 0.1, 0, 0, 0, 16, None) == _lib.ERR_ARG
    assert b"sites" in L.mgpt_last_error()


def test_dropout_flag_and_model_args():
    assert training.parse_args(REQUIRED).dropout is None               # the checkpoint's value, 0.0 for a shape name
    a = training.parse_args(REQUIRED + ["--dropout", "0.1"])
    assert a.dropout == 0.1
    with pytest.raises(SystemExit):
        training.parse_args(REQUIRED + ["--dropout", "1.0"])
    assert weights.model_args("tiny")["dropout"] == 0.0
    # the step of a micro-step: i * A + r * (A / world) + j -- two ranks of 2 micro-steps each cover one process's 4, in rank order
    one = [training.dropout_step(i, 4, 0, 1, j) for i in range(2) for j in range(4)]
    two = [training.dropout_step(i, 4, r, 2, j) for i in range(2) for r in range(2) for j in range(2)]
    assert one == two == list(range(8))


def test_dropout_kernels_use_no_scratch(tmp_path):
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
    new = {k: v for k, v in kernels.items() if "4DropE" in k or "Li7EEE" in k}      # a Drop argument, or the E_RESID_DROP epilogue
    # 3 elementwise, the fp32 forward (2 head sizes), 3 fp32 backward x 2, bf16 forward and backward x 2, the epilogue; and the p = 0 instances
    assert sum("Lb1EEEv" in k for k in new) >= 10 and len(new) >= 26, sorted(new)
    assert all(v == 0 for v in new.values()), {k: v for k, v in new.items() if v}
