"""Spread-score checkpoints for the 16-bit inference forward: the recipe, the cases and the regime figures, on the fp64 oracle alone.
Test infrastructure only (tests/test_spread_cpu.py pins it, tests/test_gpu_spread_scores.py runs it, tests/golden/make_golden_spread.py
writes the fixtures).

At N(0, 0.02) a query's scores spread by ~0.1 nat and softmax is a plain mean over the 256 keys.  Here the q and k rows of EVERY layer's
c_attn.weight are multiplied by a per-shape factor (scores grow with its square) and nothing else is touched: the MLP, wte and the LayerNorm
gains stay synthetic, logits stay of order one, and what the bars of the GPU tests see is softmax at spread scores."""
import math
import os

import numpy as np
import torch

from mapf_gpt_amd import weights
from tests.helpers import GOLDEN

# the two chains no released shape reaches: packed chain with heads of 64, generic chain
EXTRA_SHAPES = {"2x4x256": dict(n_layer=2, n_head=4, n_embd=256), "2x1x64": dict(n_layer=2, n_head=1, n_embd=64)}
CASES = ("tiny", "2M", "6M", "85M", "2x4x256", "2x1x64")

# (n_layer, n_head, n_embd) -> q/k factor, chosen on the fp64 oracle alone (tests/test_spread_cpu.py pins the conditions): on the case's
# regime rows every layer has a median per-query score spread >= 15 nats and 0.2 <= fb_lo <= fb_hi <= 0.8 (regime() below).
FACTORS = {
    (2, 2, 64): 13.0,        # tiny
    (5, 5, 160): 9.0,        # 2M
    (8, 8, 256): 7.0,        # 6M
    (12, 12, 768): 4.25,     # 85M
    (2, 4, 256): 7.0,
    (2, 1, 64): 14.0,
}
# The wpe = 0 variants of the permutation test (2M, 6M) are other functions of the tokens -- without position embeddings the first tile is no
# longer special -- so they carry factors of their own, chosen under the same conditions.
FACTORS_NOPOS = {(5, 5, 160): 9.0, (8, 8, 256): 7.0}

CALL_ROWS = 136                 # fixture rows: the first 136 of gptbig_2M_s1 tokens (the 516-row call repeats them)
CALL_ROWS_85M = 129
LARGE = 129                     # the first large call (kSmallRows = 128)
# rows on which the regime conditions hold and whose figures the fixtures store: the whole 129-row call where the fallback counter is
# bounded by them (2M, 6M), a handful elsewhere
REGIME_ROWS = {"tiny": 6, "2M": LARGE, "6M": LARGE, "85M": 2, "2x4x256": 6, "2x1x64": 6}
ROLLS = (0, 32, 96, 160)        # the permutation test's arrangements of a row's first 255 tokens
PERM_REGIME_ROWS = 8

LN_CEIL = math.log(60000.0)     # attention_tiles: a half-row sum of 60 000 sends the wave to the exact loop
BAND = 0.01                     # nats left undecided around it


def case_args(case):
    return weights.model_args(EXTRA_SHAPES.get(case, case))


def n_fixture_rows(case):
    return CALL_ROWS_85M if case == "85M" else CALL_ROWS


def tokens(n=CALL_ROWS):
    """the first n rows of the committed gptbig_2M_s1 fixture: real observation rows (every gptbig fixture holds the same 256 rows)"""
    return np.ascontiguousarray(np.load(os.path.join(GOLDEN, "gptbig_2M_s1.npz"))["tokens"][:n])


def rolled(tok, r):
    """every row's first 255 tokens rolled by r positions; the last token (the query whose logits are read) stays"""
    out = np.array(tok, copy=True)
    out[:, :255] = np.roll(tok[:, :255], r, axis=1)
    return out


def spread_state_dict(name_or_args, seed=0, factor=None, nopos=False):
    """synthetic_state_dict with the q and k rows of every layer's c_attn.weight (the last included) multiplied by the shape's factor;
    nopos: transformer.wpe.weight zeroed as well (the permutation test) and the factor taken from FACTORS_NOPOS."""
    a = weights.model_args(EXTRA_SHAPES.get(name_or_args, name_or_args) if isinstance(name_or_args, str) else name_or_args)
    L, C = a["n_layer"], a["n_embd"]
    if factor is None:
        factor = (FACTORS_NOPOS if nopos else FACTORS)[(L, a["n_head"], C)]
    sd = {k: np.array(v, dtype=np.float32) for k, v in weights.synthetic_state_dict(a, seed=seed).items()}
    for l in range(L):
        sd[f"transformer.h.{l}.attn.c_attn.weight"][:2 * C] *= np.float32(factor)
    if nopos:
        sd["transformer.wpe.weight"][:] = 0
    sd["lm_head.weight"] = sd["transformer.wte.weight"]
    return sd


def _scores(sd, args, tok, chunk=32):
    """fp64 scores of the oracle port, chunk rows at a time: yields (first row, [per layer: s [rows, heads, 256 queries, 256 keys] in nats])"""
    import torch.nn.functional as F
    from oracle import gpt_oracle
    w = gpt_oracle.to_torch(sd, torch.float64)
    nh, C = args["n_head"], args["n_embd"]
    tok = np.asarray(tok)
    for r0 in range(0, len(tok), chunk):
        xs = gpt_oracle.forward_logits(sd, args, tok[r0:r0 + chunk], dtype=torch.float64, return_layers=True)[1]
        out = []
        for l in range(args["n_layer"]):
            p, x = f"transformer.h.{l}.", xs[l]
            B, T, _ = x.shape
            qkv = F.linear(F.layer_norm(x, (C,), w[p + "ln_1.weight"], None, 1e-5), w[p + "attn.c_attn.weight"])
            q, k, _ = (t.view(B, T, nh, C // nh).transpose(1, 2) for t in qkv.split(C, dim=2))
            out.append(q @ k.transpose(-1, -2) / (C // nh) ** 0.5)
        yield r0, out


def verdicts(sd, args, tok):
    """fp64, per layer: (spread [rows, heads, 256] = max - min score of every query,
                         must [rows, heads, 8] bool: some query of the block of 32 consecutive queries has a score more than
                              ln 60000 + BAND above the maximum of its first 32 keys -- p = exp(s - reference) then exceeds the fp16 ceiling of
                              the P planes in whichever half-row holds that key, and the wave must fall back,
                         stay [rows, heads, 8] bool: every query of the block has sum_j exp(s_j - reference) < 60000 e^-BAND -- both half-row
                              sums are below the ceiling, and the wave must stay on the pipelined loop)"""
    L = args["n_layer"]
    acc = [([], [], []) for _ in range(L)]
    for _, layers in _scores(sd, args, tok):
        for l, s in enumerate(layers):
            B, nh, T, _ = s.shape
            ref = s[..., :32].max(-1).values
            must_q = (s.max(-1).values - ref) > LN_CEIL + BAND
            stay_q = torch.logsumexp(s - ref[..., None], -1) < LN_CEIL - BAND
            acc[l][0].append((s.max(-1).values - s.min(-1).values).numpy())
            acc[l][1].append(must_q.view(B, nh, T // 32, 32).any(-1).numpy())
            acc[l][2].append(stay_q.view(B, nh, T // 32, 32).all(-1).numpy())
    return [tuple(np.concatenate(a) for a in layer) for layer in acc]


def regime(sd, args, tok):
    """fp64, per layer: (median over the queries of every row and head of max - min score in nats,
                         fb_lo = share of (row, head, block of 32 queries) that MUST fall back,
                         fb_hi = 1 - share of blocks that MUST stay on the pipelined loop)      -- see verdicts()"""
    return [(float(np.median(sp)), float(must.mean()), float(1.0 - stay.mean())) for sp, must, stay in verdicts(sd, args, tok)]


def changed_share(sd, args, tok, rolls=ROLLS):
    """The permutation test's condition, over layers 0 .. L-2 (the layers the persistent kernels run in a last-position call).
    -> (share of (layer, row, head) whose eight per-wave must-fall-back verdicts differ between two arrangements,
        share of single (layer, row, head, wave) verdicts that differ between two arrangements)"""
    L = args["n_layer"]
    must = [np.stack([v[1] for v in verdicts(sd, args, rolled(tok, r))[:L - 1]]) for r in rolls]      # each [L-1, rows, heads, 8]
    diff = np.zeros(must[0].shape, bool)
    for i in range(len(must)):
        for j in range(i + 1, len(must)):
            diff |= must[i] != must[j]
    return float(diff.any(-1).mean()), float(diff.mean())


def load_fixture(case):
    return np.load(os.path.join(GOLDEN, f"gptspread_{case}.npz"))
