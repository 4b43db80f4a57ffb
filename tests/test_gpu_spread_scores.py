"""The 16-bit inference forward at SPREAD softmax scores (tests/spread_ref.py: q and k rows of every layer scaled until a query's scores
spread by 20-30 nats, as a trained checkpoint's do) against the real model.py's fp64 logits (tests/golden/gptspread_<case>.npz).

At N(0, 0.02) every attention kernel rescales with alpha ~ 1 and sums p ~ 1; here alpha << 1, probabilities underflow the fp16 P planes, the
pipelined loop of attention_tiles (gpt_kernels_attn_tiles.h) runs with p up to its 60 000 ceiling and 25-50 % of its waves redo their head
with attention_exact_tiles -- inside one launch, in all four instantiations (attn256q_kernel / attn160o_kernel, split fp16 / bf16).

Cases: the smallest calls that reach each kernel (129 rows is the first large call, kSmallRows = 128):
    tiny (2x2x64)   3, 129      attn_block head-parallel + one-launch tail; attn_block row-per-workgroup with fused embedding + attn_last1
    2M              3, 129      head-parallel + tail; attn160o pipelined + fallback, table embedding, attn_last1
    6M              3, 129, 516 attn256_kernel<HP> + tail; attn256q pipelined + fallback, layer-0 table, attn_last1 one row per workgroup;
                                516 rows > 2 x 256 CUs: attn_last1 with kLast1R rows per workgroup
    85M             3, 129      attn16_kernel, 128-row GEMM tiles; LAST_PACKED
    2x4x256         3, 129      packed chain with heads of 64
    2x1x64          3, 129      generic chain
Bars, with e32 = max|logits_f32 - logits_f64| and e16 = max|logits_bf16 - logits_f64| of the fixture (the reference's own errors):
    f32     max|dev - f64| <= max(1e-5, 3 e32)       ("as close to fp64 as torch's own fp32", test_envelope_bar_is_relative_once_the_logits_are_large)
    f16x3   max|dev - f64| <= max(1e-5, 64 2^-23 max|logits_f64|, 8 e32)
            (the library's probe bar MGPT_ENVELOPE_PROBE_TOL / _REL; 8 = 4 x the unit round-off of 22 against 24 significant bits per
             operand, x 2 for the other summation order -- not measured)
    bf16    max|dev - f64| <= 1.5 e16 + 2e-3, max|dev - autocast| <= 2.5 e16 + 2e-3, and > 1e-6     (test_bf16_mode_vs_reference_autocast's bars)
Every measured figure goes to record_parity(test="spread_scores", ...)."""
import functools

import numpy as np
import pytest
import torch

from mapf_gpt_amd import _lib
from tests import spread_ref
from tests.helpers import record_parity
from tests.test_loss_cpu import seq_oracle

pytestmark = pytest.mark.gpu

PROBE_TOL, PROBE_REL = 1e-5, 7.62939453125e-6     # include/mapf_gpt_amd.h MGPT_ENVELOPE_PROBE_TOL / _REL (64 * 2^-23)
CALLS = [("tiny", 3), ("tiny", 129), ("2M", 3), ("2M", 129), ("6M", 3), ("6M", 129), ("6M", 516), ("85M", 3), ("85M", 129),
         ("2x4x256", 3), ("2x4x256", 129), ("2x1x64", 3), ("2x1x64", 129)]
MAX_ROWS = {case: max(n for c, n in CALLS if c == case) for case in spread_ref.CASES}
COUNTED = ("2M", "6M")                            # the shapes whose large calls run attention_tiles (the fallback counter)


@functools.lru_cache(maxsize=None)
def _case(case, nopos=False):
    """one model per case (max_rows = its largest call, every precision by argument), its state dict, args and fixture"""
    from mapf_gpt_amd.model import build_model
    args = spread_ref.case_args(case)
    sd = spread_ref.spread_state_dict(case, nopos=nopos)
    g = spread_ref.load_fixture(case + ("_nopos" if nopos else ""))
    assert float(g["factor"]) == (spread_ref.FACTORS_NOPOS if nopos else spread_ref.FACTORS)[(args["n_layer"], args["n_head"], args["n_embd"])]
    # (the scaled weights lie outside the weight-statistics envelope: "ignore" runs the split path regardless, and conftest's autouse
    #  fixture fails the test if an f16x3 request were served in fp32 after all)
    net = build_model(args, precision="f16x3", max_rows=spread_ref.LARGE if nopos else MAX_ROWS[case], state_dict=sd, envelope="ignore")
    return net, sd, args, {k: g[k] for k in g.files}


def _bars(g, rows, precision):
    """-> (bar against logits_f64, bar against logits_bf16 or None, e32, e16): from the fixture alone, over the rows of the call"""
    f64 = g["logits_f64"][rows]
    e32 = float(np.abs(g["logits_f32"][rows] - f64).max())
    e16 = float(np.abs(g["logits_bf16"][rows] - f64).max())
    if precision == "f32":
        return max(1e-5, 3.0 * e32), None, e32, e16
    if precision == "f16x3":
        return max(PROBE_TOL, PROBE_REL * float(np.abs(f64).max()), 8.0 * e32), None, e32, e16
    return 1.5 * e16 + 2e-3, 2.5 * e16 + 2e-3, e32, e16


def _counter_bounds(g, layers, N):
    lo, hi = float(np.mean(g["fb_lo"][:layers])), float(np.mean(g["fb_hi"][:layers]))
    return lo * N - 0.01 * N, hi * N + 0.01 * N


def _call_tokens(case, n):
    base = spread_ref.tokens(spread_ref.n_fixture_rows(case))
    idx = np.arange(n) % len(base)                # (the 516-row call repeats the 136 fixture rows)
    return np.ascontiguousarray(base[idx]), idx


@pytest.mark.parametrize("precision", ["f32", "f16x3", "bf16"])
@pytest.mark.parametrize("case,n", CALLS)
def test_spread_logits_vs_reference_fp64(case, n, precision):
    net, _, args, g = _case(case)
    tok_np, idx = _call_tokens(case, n)
    tok = torch.from_numpy(tok_np).cuda()
    f64 = g["logits_f64"][idx]
    bar, bar_mut, e32, e16 = _bars(g, idx, precision)
    got = net.logits_tokens(tok, precision=precision).cpu().numpy().astype(np.float64)     # (the first f16x3 call also runs the envelope probe)
    greedy = net.act_tokens(tok, do_sample=False, precision=precision).cpu().numpy()
    _lib.debug_counter(0, reset=True)
    again = net.logits_tokens(tok, precision=precision).cpu().numpy().astype(np.float64)
    count = _lib.debug_counter(0, reset=True)
    err = float(np.abs(got - f64).max())
    top2 = np.sort(f64[:, :5], axis=1)[:, -2:]
    safe = (top2[:, 1] - top2[:, 0]) > 4 * bar                   # arg-max may legitimately flip only inside the bar
    rec = dict(test="spread_scores", kind="last", shape=case, rows=n, precision=precision, factor=float(g["factor"]), err_vs_fp64=err, bar=bar, e32=e32,
               e16=e16, max_abs_logit=float(np.abs(f64).max()), fallbacks=count, greedy_rows_checked=int(safe.sum()))
    if precision == "bf16":
        rec.update(err_vs_autocast=float(np.abs(got - g["logits_bf16"][idx]).max()), bar_vs_autocast=bar_mut)
    N = n * args["n_head"] * 8 * (args["n_layer"] - 1)           # (row, head, wave) of layers 0 .. L-2: the last layer is attn_last1
    if case in COUNTED and n > 128 and precision != "f32":
        rec.update(N=N)
        if n == spread_ref.LARGE and precision == "f16x3":
            rec["count_lo"], rec["count_hi"] = _counter_bounds(g, args["n_layer"] - 1, N)
    record_parity(**rec)
    print(rec)
    assert np.isfinite(got).all()
    assert np.array_equal(got, again), "two calls of the same rows differ"
    assert err <= bar, f"{case} {precision} {n} rows: max |dev - fp64| = {err:.3e}, bar {bar:.3e} (e32 {e32:.2e}, e16 {e16:.2e})"
    if precision == "bf16":
        assert rec["err_vs_autocast"] <= bar_mut, f"{case} bf16 {n} rows: max |dev - autocast| = {rec['err_vs_autocast']:.3e}, bar {bar_mut:.3e}"
        assert err > 1e-6, "this must be the reduced-precision path"
    assert np.array_equal(greedy[safe], np.argmax(f64[:, :5], axis=1)[safe])
    if case in COUNTED and precision != "f32":
        if n <= 128:
            assert count == 0, f"{case} {precision}: a small call does not run attention_tiles, counter {count}"
        elif precision == "bf16" or n != spread_ref.LARGE:
            assert 0 < count < N, f"{case} {precision} {n} rows: {count} fallbacks of {N}"      # bf16 scores round by ~0.1 nat: no sharper bound
        else:
            # an f16x3 score is within ~3e-5 nat of fp64 at 30 nats, far inside the 0.01-nat band regime() leaves undecided; 1 % slack is a cap
            assert rec["count_lo"] <= count <= rec["count_hi"], f"{case} f16x3: {count} fallbacks of {N}, expected {rec['count_lo']:.0f} .. {rec['count_hi']:.0f}"


@pytest.mark.parametrize("case", COUNTED)
def test_spread_sequence_forward_every_position(case):
    """net(idx, targets) in f16x3 on 129 rows: the last layer runs as a full layer, so the persistent kernel and its fallback serve it too
    (counter over all L layers).  Rows {0, 1, 128} at every position against seq_oracle in fp64 (bar 2 with e32 from seq_oracle in fp32 on the
    same rows); only these rows carry targets, so the call's loss is theirs (1e-4 relative, test_gpu_loss.py's figure)."""
    net, sd, args, g = _case(case)
    n, cmp = spread_ref.LARGE, np.array([0, 1, 128])
    tok = spread_ref.tokens(n)
    rng = np.random.Generator(np.random.PCG64(17))
    tg = np.full((n, 256), -1, np.int64)
    tg[cmp] = rng.integers(0, 67, (3, 256))
    tg[1, rng.random(256) < 0.3] = -1
    net.logits_tokens(torch.from_numpy(tok).cuda())                # (decides the envelope outside the counted call)
    _lib.debug_counter(0, reset=True)
    logits, loss = net(torch.from_numpy(tok).cuda(), torch.from_numpy(tg).cuda())
    logits, loss = logits.cpu().numpy().astype(np.float64), float(loss)
    count = _lib.debug_counter(0, reset=True)
    ref64, loss64 = seq_oracle(sd, args, tok[cmp], tg[cmp], dtype=torch.float64)
    ref32, _ = seq_oracle(sd, args, tok[cmp], None, dtype=torch.float32)
    ref64 = ref64.numpy()
    e32 = float(np.abs(ref32.numpy().astype(np.float64) - ref64).max())
    bar = max(PROBE_TOL, PROBE_REL * float(np.abs(ref64).max()), 8.0 * e32)
    err = float(np.abs(logits[cmp] - ref64).max())
    N = n * args["n_head"] * 8 * args["n_layer"]
    lo, hi = _counter_bounds(g, args["n_layer"], N)
    rec = dict(test="spread_scores", kind="seq", shape=case, rows=n, precision="f16x3", factor=float(g["factor"]), err_vs_fp64=err, bar=bar, e32=e32,
               max_abs_logit=float(np.abs(ref64).max()), loss=loss, loss_fp64=float(loss64), fallbacks=count, N=N, count_lo=lo, count_hi=hi)
    record_parity(**rec)
    print(rec)
    assert np.isfinite(logits).all()
    assert err <= bar, f"{case}: logits of every position differ by {err:.3e} (bar {bar:.3e}, e32 {e32:.2e})"
    assert abs(loss - float(loss64)) <= 1e-4 * abs(float(loss64)), (case, loss, float(loss64))
    assert lo <= count <= hi, f"{case}: {count} fallbacks of {N}, expected {lo:.0f} .. {hi:.0f}"


@pytest.mark.parametrize("precision", ["f16x3", "bf16"])
@pytest.mark.parametrize("case", COUNTED)
def test_pipelined_loop_against_exact_loop_by_a_permutation(case, precision):
    """model.py's attention has no mask, so with wpe = 0 a row's logits at position 255 depend only on its last token and the multiset of the
    other 255.  Rolling a row's first 255 tokens by 32, 96 and 160 positions changes which keys form the first tile, with them the softmax
    reference of every query and which waves fall back (tests/test_spread_cpu.py: more than 10 % of the waves change their verdict) -- the
    four logit sets must agree pairwise within twice the case's bar, and each lies within the bar of the reference's fp64 logits of the unrolled
    rows.  With wpe kept the roll changes the function: the oracle's logits then move by more than 1e-3 (asserted in test_spread_cpu.py),
    and on the device, checked once, the four arrangements of the wpe-carrying checkpoints differ pairwise by 1.03 (2M) and 1.40 (6M) in
    either precision, against bars of 4e-5 .. 0.1: without wpe = 0 this test fails."""
    net, _, args, g = _case(case, nopos=True)
    n = spread_ref.LARGE
    tok = spread_ref.tokens(n)
    idx = np.arange(n)
    bar, _, e32, e16 = _bars(g, idx, precision)
    outs, counts = [], []
    net.logits_tokens(torch.from_numpy(tok).cuda(), precision=precision)
    for r in spread_ref.ROLLS:
        _lib.debug_counter(0, reset=True)
        outs.append(net.logits_tokens(torch.from_numpy(spread_ref.rolled(tok, r)).cuda(), precision=precision).cpu().numpy().astype(np.float64))
        counts.append(_lib.debug_counter(0, reset=True))
    pair = max(float(np.abs(outs[i] - outs[j]).max()) for i in range(4) for j in range(i + 1, 4))
    err = max(float(np.abs(o - g["logits_f64"][idx]).max()) for o in outs)
    N = n * args["n_head"] * 8 * (args["n_layer"] - 1)
    rec = dict(test="spread_scores", kind="permutation", shape=case, rows=n, precision=precision, factor=float(g["factor"]), pairwise=pair, err_vs_fp64=err,
               bar=bar, e32=e32, e16=e16, max_abs_logit=float(np.abs(g["logits_f64"][idx]).max()), fallbacks=counts, N=N)
    record_parity(**rec)
    print(rec)
    assert all(np.isfinite(o).all() for o in outs)
    assert all(0 < c < N for c in counts) and len(set(counts)) > 1, f"the rolls were meant to move the fallback decisions: {counts} of {N}"
    assert pair <= 2 * bar, f"{case} {precision}: arrangements differ by {pair:.3e}, bar 2 x {bar:.3e}"
    assert err <= bar, f"{case} {precision}: max |dev - fp64| = {err:.3e} over the arrangements, bar {bar:.3e}"
