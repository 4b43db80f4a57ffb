"""The last-position micro-step with dropout without a GPU: the math its kernels implement (tests/train_rows_dropout_ref.py: the compact last
layer with masks and a hand-written backward) against fp64 autograd of the masked general restatement on last-only targets, the compact
mask indices against the general call's at token / query 255, the C binding and the --rows-call-drop flag of the training CLI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from mapf_gpt_amd import _lib, training, weights
from mapf_gpt_amd.sampling import dropout_keep
from tests import train_dropout_ref as tdr
from tests.helpers import ROOT
from tests.train_ref import LOCALISERS, expert_rows, targets_last, trained_like_state_dict
from tests.train_rows_dropout_ref import compact_index, loss_and_grads_rows_drop

SEED, STEP = 11, 3


def _case(name, rows):
    args = weights.model_args(LOCALISERS.get(name, name))
    tokens, labels = expert_rows(rows, seed=len(name))
    return args, trained_like_state_dict(args), tokens, labels


@pytest.mark.parametrize("sites", [1, 2, 4, 8, 15], ids=["embedding", "attention", "attn_proj", "mlp_proj", "all"])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("name", ["tiny", *LOCALISERS])
def test_compact_last_layer_with_masks_matches_fp64_autograd(name, p, rows, sites):
    """both sides fp64 with the same masks, differing by rounding only: the loss and every gradient within 1e-9 max|g|"""
    args, sd, tokens, labels = _case(name, rows)
    l_ref, g_ref = tdr.loss_and_grads(sd, args, tokens, targets_last(labels), p, SEED, STEP, row0=2, sites=sites)
    loss, got = loss_and_grads_rows_drop(sd, args, tokens, labels, p, SEED, STEP, row0=2, sites=sites)
    assert abs(loss - l_ref) <= 1e-9 * abs(l_ref), (loss, l_ref)
    assert set(got) == set(g_ref)
    for k, ref in g_ref.items():
        m = float(ref.abs().max())
        err = float((got[k] - ref).abs().max())
        assert err <= 1e-9 * m, f"{name} {k}: max|g - g64| {err:.3e}, max|g64| {m:.3e}"


def test_masks_change_the_gradients():
    """(the comparison above is not one of two dropout-free runs)"""
    args, sd, tokens, labels = _case("1x2x64", 3)
    _, g0 = loss_and_grads_rows_drop(sd, args, tokens, labels, 0.0, SEED, STEP)
    for sites in (1, 2, 4, 8):
        _, g = loss_and_grads_rows_drop(sd, args, tokens, labels, 0.5, SEED, STEP, sites=sites)
        k = "transformer.h.0.attn.c_attn.weight"
        assert float((g[k] - g0[k]).abs().max()) > 1e-3 * float(g0[k].abs().max()), sites


@pytest.mark.parametrize("row0", [0, 5])
@pytest.mark.parametrize("name", ["tiny", *LOCALISERS])
def test_compact_mask_indices_are_the_general_calls_at_token_255(name, row0):
    args = weights.model_args(LOCALISERS.get(name, name))
    nh, C, L, rows, p = args["n_head"], args["n_embd"], args["n_layer"], 3, 0.5
    r = row0 + np.arange(rows, dtype=np.uint64)
    # site 1: ((row0 + row) n_head + head) 65536 + query 256 + key at query 255
    general = ((r[:, None, None, None] * nh + np.arange(nh, dtype=np.uint64)[None, :, None, None]) * 65536
               + np.arange(256, dtype=np.uint64)[None, None, :, None] * 256 + np.arange(256, dtype=np.uint64)[None, None, None, :])
    assert np.array_equal(compact_index(tdr.SITE_ATTN, args, row0, rows), general[:, :, 255, :])
    full = tdr.factor(SEED, STEP, tdr.SITE_ATTN, L - 1, p, row0, rows, args, "cpu").numpy() > 0
    assert np.array_equal(dropout_keep(SEED, STEP, tdr.SITE_ATTN, L - 1, compact_index(tdr.SITE_ATTN, args, row0, rows), p), full[:, :, 255, :])
    # sites 2, 3: ((row0 + row) 256 + t) C + c at t = 255
    general = (r[:, None, None] * 256 + np.arange(256, dtype=np.uint64)[None, :, None]) * C + np.arange(C, dtype=np.uint64)[None, None, :]
    for site in (tdr.SITE_ATTN_PROJ, tdr.SITE_MLP_PROJ):
        assert np.array_equal(compact_index(site, args, row0, rows), general[:, 255, :])
        full = tdr.factor(SEED, STEP, site, L - 1, p, row0, rows, args, "cpu").numpy() > 0
        assert np.array_equal(dropout_keep(SEED, STEP, site, L - 1, compact_index(site, args, row0, rows), p), full[:, 255, :])
    # the kernels' form of site 1: one hash per four consecutive keys, hash counter (base >> 2) + bh * 16384 + ((255 * 256 + j) >> 2), slot j & 3
    idx = compact_index(tdr.SITE_ATTN, args, row0, rows)
    bh = (r[:, None] * nh + np.arange(nh, dtype=np.uint64)[None, :])[:, :, None]
    j = np.arange(256, dtype=np.uint64)[None, None, :]
    assert np.array_equal(idx >> np.uint64(2), bh * np.uint64(16384) + ((np.uint64(255 * 256) + j) >> np.uint64(2)))
    assert np.array_equal(idx & np.uint64(3), np.broadcast_to(j & np.uint64(3), idx.shape))


def test_forward_backward_rows_drop_binding_and_argument_checks():
    src = open(os.path.join(ROOT, "include", "mapf_gpt_amd.h")).read()
    decl = re.search(r"int mgpt_gpt_forward_backward_rows_drop\((.*?)\);", src, flags=re.S)
    assert decl is not None and len(decl.group(1).split(",")) == 13
    res, args = _lib.SYMBOLS["mgpt_gpt_forward_backward_rows_drop"]
    assert res is ctypes.c_int and len(args) == 13 and args[7] is ctypes.c_float and args[8] is ctypes.c_uint64
    assert args[:7] == _lib.SYMBOLS["mgpt_gpt_forward_backward_rows"][1][:7]
    from mapf_gpt_amd import build
    build.build()
    L = _lib.lib()
    for p in (1.0, -0.1, float("nan")):
        assert L.mgpt_gpt_forward_backward_rows_drop(None, None, 1, None, 1.0, None, _lib.PREC_F32, p, 0, 0, 0, 15, None) == _lib.ERR_ARG
        assert b"dropout p" in L.mgpt_last_error()
    assert L.mgpt_gpt_forward_backward_rows_drop(None, None, 1, None, 1.0, None, _lib.PREC_F32, 0.1, 0, 0, 0, 16, None) == _lib.ERR_ARG
    assert b"sites" in L.mgpt_last_error()
    assert L.mgpt_gpt_forward_backward_rows_drop(None, None, 1, None, 1.0, None, _lib.PREC_F32, 0.1, 0, 0, 0, 15, None) == _lib.ERR_ARG     # NULL model


def test_rows_call_drop_flag():
    base = ["--init", "tiny", "--data", "d", "--val", "v"]
    assert training.parse_args(base).rows_call_drop is False
    a = training.parse_args(base + ["--rows-call-drop", "--dropout", "0.1"])
    assert a.rows_call_drop is True and a.rows_call is False and a.dropout == 0.1
    a = training.parse_args(base + ["--rows-call-drop"])
    assert a.rows_call_drop is True and a.dropout is None           # the checkpoint's value, whatever it is
    assert training.parse_args(base + ["--rows-call-drop", "--dropout", "0"]).rows_call_drop is True
    with pytest.raises(SystemExit):                                  # --rows-call is what it was
        training.parse_args(base + ["--rows-call", "--dropout", "0.1"])
    with pytest.raises(SystemExit):
        training.parse_args(base + ["--rows-call", "--rows-call-drop"])
