"""Conditions on the INPUTS of tests/test_gpu_spread_scores.py, on the fp64 oracle alone: the spread-score recipe scales what it says and
nothing else, every case reaches its regime (both loops of attention_tiles inside one launch), the committed fixtures carry the figures
tests/spread_ref.py computes, and the permutation test's rolls really move the fallback decisions."""
import numpy as np
import pytest

from mapf_gpt_amd import weights
from tests import spread_ref

PINNED = {"tiny": 13.0, "2M": 9.0, "6M": 7.0, "85M": 4.25, "2x4x256": 7.0, "2x1x64": 14.0}
PINNED_NOPOS = {"2M": 9.0, "6M": 7.0}


def _key(a):
    return (a["n_layer"], a["n_head"], a["n_embd"])


def _check_regime(name, figures):
    for l, (spread, lo, hi) in enumerate(figures):
        assert spread >= 15.0, f"{name} layer {l}: median per-query score spread {spread:.2f} nats"
        assert 0.2 <= lo <= hi <= 0.8, f"{name} layer {l}: fb_lo {lo:.3f}, fb_hi {hi:.3f}"


@pytest.mark.parametrize("case", spread_ref.CASES)
def test_recipe_scales_q_and_k_of_every_layer_and_nothing_else(case):
    a = spread_ref.case_args(case)
    f = spread_ref.FACTORS[_key(a)]
    assert f == PINNED[case]
    sd, base = spread_ref.spread_state_dict(case), weights.synthetic_state_dict(a, seed=0)
    C = a["n_embd"]
    assert set(sd) == set(base) and all(sd[k].shape == base[k].shape and sd[k].dtype == np.float32 for k in base)
    for k in base:
        if k.endswith("attn.c_attn.weight"):
            assert np.array_equal(sd[k][:2 * C], base[k][:2 * C] * np.float32(f)) and np.array_equal(sd[k][2 * C:], base[k][2 * C:]), k
        else:
            assert np.array_equal(sd[k], base[k]), k
    assert sum(k.endswith("attn.c_attn.weight") for k in base) == a["n_layer"]
    assert np.array_equal(sd["lm_head.weight"], sd["transformer.wte.weight"])


@pytest.mark.parametrize("case", spread_ref.CASES)
def test_spread_recipe_reaches_its_regime_and_the_fixture_says_so(case):
    """Every layer: median spread >= 15 nats and 0.2 <= fb_lo <= fb_hi <= 0.8 on the case's regime rows; the fixture stores exactly these
    figures (the GPU test bounds the fallback counter by them) together with the factor and the seed."""
    a = spread_ref.case_args(case)
    g = spread_ref.load_fixture(case)
    n = spread_ref.REGIME_ROWS[case]
    assert float(g["factor"]) == spread_ref.FACTORS[_key(a)] and int(g["seed"]) == 0 and int(g["regime_rows"]) == n
    figures = spread_ref.regime(spread_ref.spread_state_dict(case), a, spread_ref.tokens(n))
    _check_regime(case, figures)
    got = np.array(figures)
    for j, key in enumerate(("spread", "fb_lo", "fb_hi")):
        assert g[key].shape == (a["n_layer"],) and np.abs(g[key] - got[:, j]).max() <= 1e-9, (case, key, g[key], got[:, j])
    rows = spread_ref.n_fixture_rows(case)
    assert g["logits_f32"].shape == g["logits_f64"].shape == g["logits_bf16"].shape == (rows, 67)
    assert g["logits_f64"].dtype == np.float64 and np.isfinite(g["logits_f64"]).all()
    assert set(g.files) == {"factor", "seed", "regime_rows", "spread", "fb_lo", "fb_hi", "logits_f32", "logits_f64", "logits_bf16"}   # no tokens, no weights


@pytest.mark.parametrize("case", ["2M", "6M"])
def test_fixture_logits_are_the_oracle_ports(case):
    """the fixtures come from the real model.py; the pinned oracle port gives the same fp64 logits on the regenerated tokens and weights
    (so the seeds and the row choice a test regenerates are the generator's)"""
    import torch
    from oracle import gpt_oracle
    g = spread_ref.load_fixture(case)
    rows = np.array([0, 1, 128, 135])
    ref = gpt_oracle.forward_logits(spread_ref.spread_state_dict(case), spread_ref.case_args(case), spread_ref.tokens()[rows], dtype=torch.float64).numpy()
    assert np.abs(ref - g["logits_f64"][rows]).max() <= 1e-11


@pytest.mark.parametrize("case", ["2M", "6M"])
def test_permutation_rolls_move_the_fallback_decisions(case):
    """wpe = 0 checkpoints of the permutation test: the regime holds on their rows, position 255's logits are invariant under a roll of the
    first 255 tokens on the oracle (and NOT with wpe kept), and between two of the four arrangements at least 10 % of the (layer, row, head)
    triples -- and of the single waves -- change their must-fall-back verdict."""
    import torch
    from oracle import gpt_oracle
    a = spread_ref.case_args(case)
    assert spread_ref.FACTORS_NOPOS[_key(a)] == PINNED_NOPOS[case]
    g = spread_ref.load_fixture(case + "_nopos")
    sd = spread_ref.spread_state_dict(case, nopos=True)
    assert not sd["transformer.wpe.weight"].any()
    tok = spread_ref.tokens(spread_ref.PERM_REGIME_ROWS)
    figures = spread_ref.regime(sd, a, tok)
    _check_regime(case + " wpe=0", figures)
    assert float(g["factor"]) == PINNED_NOPOS[case] and np.abs(np.array(figures) - np.stack([g["spread"], g["fb_lo"], g["fb_hi"]], 1)).max() <= 1e-9
    pairs, waves = spread_ref.changed_share(sd, a, tok)
    assert pairs >= 0.10 and waves >= 0.10, f"{case}: {pairs:.3f} of the (layer, row, head) triples, {waves:.3f} of the waves change their verdict"
    ref = [gpt_oracle.forward_logits(sd, a, spread_ref.rolled(tok[:2], r), dtype=torch.float64).numpy() for r in spread_ref.ROLLS]
    assert max(np.abs(r - ref[0]).max() for r in ref[1:]) <= 1e-12
    sdp = spread_ref.spread_state_dict(case)
    with_pos = [gpt_oracle.forward_logits(sdp, a, spread_ref.rolled(tok[:2], r), dtype=torch.float64).numpy() for r in spread_ref.ROLLS[:2]]
    assert np.abs(with_pos[1] - with_pos[0]).max() > 1e-3, "with wpe kept the roll changes the function"
