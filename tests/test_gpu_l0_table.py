"""Layer 0 of the 6M shape from the per-checkpoint (position, token) table of q | k | v (attn256q_kernel<.., TAB = 2>).

The table is built by the EMB kernel itself on synthetic rows, so a large call must give the same bits with the table as without it
(MGPT_L0_TABLE=0, read when a precision mode is built: at a model's first forward in that mode)."""
import contextlib
import os

import numpy as np
import pytest
import torch

from mapf_gpt_amd import _lib, weights
from mapf_gpt_amd.model import build_model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _table(on):
    old = os.environ.get("MGPT_L0_TABLE")
    if on:
        os.environ.pop("MGPT_L0_TABLE", None)
    else:
        os.environ["MGPT_L0_TABLE"] = "0"
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("MGPT_L0_TABLE", None)
        else:
            os.environ["MGPT_L0_TABLE"] = old


def _twins(precision, max_rows, seed=0, state_dict=None, envelope="fallback"):
    """(with table, without table): each mode is built by the first forward, inside the environment it is meant to see"""
    probe = torch.zeros((1, 256), dtype=torch.uint8, device="cuda")
    nets = []
    for on in (True, False):
        with _table(on):
            net = build_model("6M", seed=seed, max_rows=max_rows, precision=precision, state_dict=state_dict, envelope=envelope)
            net.logits_tokens(probe)
        nets.append(net)
    return nets


def _rows(n, seed=0):
    base = np.load(os.path.join(GOLDEN, "gptbig_6M_s1.npz"))["tokens"]
    rng = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(np.ascontiguousarray(base[rng.integers(0, len(base), n)])).cuda()


def _same(a, b, tok):
    la, lb = a.logits_tokens(tok).cpu().numpy(), b.logits_tokens(tok).cpu().numpy()
    assert np.isfinite(la).all()
    assert np.array_equal(la, lb), f"max |dlogit| = {np.abs(la - lb).max():.3e}"
    assert torch.equal(a.act_tokens(tok, do_sample=False), b.act_tokens(tok, do_sample=False))
    assert torch.equal(a.act_tokens(tok, do_sample=True, seed=7, step=3), b.act_tokens(tok, do_sample=True, seed=7, step=3))


@pytest.mark.parametrize("rows", [512, 12288])
@pytest.mark.parametrize("precision", ["f16x3", "bf16"])
def test_table_is_bit_identical_to_the_embedding_path(precision, rows):
    on, off = _twins(precision, rows)
    _same(on, off, _rows(rows))


@pytest.mark.parametrize("precision", ["f16x3", "bf16"])
def test_every_position_token_pair(precision):
    """the table's own synthetic rows (row j = token j at every position), three times over: a large call (> 128 rows)"""
    syn = np.repeat(np.arange(67, dtype=np.uint8)[:, None], 256, axis=1)
    tok = torch.from_numpy(np.ascontiguousarray(np.concatenate([syn, syn[::-1], np.roll(syn, 5, axis=0)]))).cuda()
    on, off = _twins(precision, tok.shape[0])
    _same(on, off, tok)


def test_exact_fallback_of_the_attention_phase():
    """layer 0's q and k rows scaled until the pipelined key-tile loop throws heads away (the exact loop redoes them): still bit-identical"""
    sd = weights.synthetic_state_dict("6M", seed=0)
    sd["transformer.h.0.attn.c_attn.weight"][:512] *= 7.0
    on, off = _twins("f16x3", 256, state_dict=sd, envelope="ignore")
    tok = _rows(256, seed=1)
    _lib.debug_counter(0, reset=True)
    la = on.logits_tokens(tok).cpu().numpy()
    assert _lib.debug_counter(0, reset=True) > 0, "the scaled layer 0 was meant to leave the fp16 range of the P planes somewhere"
    lb = off.logits_tokens(tok).cpu().numpy()
    assert _lib.debug_counter(0, reset=True) > 0
    assert np.array_equal(la, lb), f"max |dlogit| = {np.abs(la - lb).max():.3e}"


def test_two_checkpoints_keep_their_own_tables():
    a_on, a_off = _twins("f16x3", 256, seed=0)
    b_on, b_off = _twins("f16x3", 256, seed=1)
    tok = _rows(256, seed=2)
    la, lb = a_on.logits_tokens(tok).cpu().numpy(), b_on.logits_tokens(tok).cpu().numpy()
    assert np.abs(la - lb).max() > 1e-3                    # (different checkpoints)
    assert np.array_equal(la, a_off.logits_tokens(tok).cpu().numpy())
    assert np.array_equal(lb, b_off.logits_tokens(tok).cpu().numpy())
    assert np.array_equal(la, a_on.logits_tokens(tok).cpu().numpy())
