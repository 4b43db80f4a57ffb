"""Policy forward parity: HIP kernels vs the reference's golden logits (real model.py, synthetic weights) and
vs the fp32/fp64 torch port, through the C ABI.  Tolerance: 1e-5 on logits (BASELINE.json north_star)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from mapf_gpt_amd import _lib, sampling, weights
from oracle import gpt_oracle
from tests.helpers import GOLDEN, load_tok

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _net(name, scale=1.0, max_rows=16, seed=0):
    from mapf_gpt_amd.model import build_model
    return build_model(name, seed=seed, scale=scale, max_rows=max_rows)


@pytest.mark.parametrize("tag", ["tiny_s1", "tiny_s4", "2M_s1", "2M_s4", "6M_s1", "85M_s1"])
def test_f32_logits_match_reference_golden(tag):
    g = np.load(os.path.join(GOLDEN, f"gpt_{tag}.npz"))
    name = tag.split("_")[0]
    net = _net(name, scale=float(g["scale"]))
    tokens = torch.from_numpy(g["tokens"]).cuda()
    logits = net.logits_tokens(tokens).cpu().numpy()
    err = np.abs(logits - g["logits"]).max()
    assert err <= TOL, f"{tag}: max |dlogit| = {err:.3e}"
    greedy = net.act_tokens(tokens, do_sample=False).cpu().numpy()
    # arg-max may legitimately flip only where the top-2 gap is inside the tolerance
    top2 = np.sort(g["logits"][:, :5], axis=1)[:, -2:]
    safe = (top2[:, 1] - top2[:, 0]) > 4 * TOL
    assert np.array_equal(greedy[safe], g["greedy"][safe])


def test_single_layer_stages_vs_fp64():
    """L=1 model: check q|k|v, MLP hidden and the residual stream separately against an fp64 port (localises a
    wrong kernel: LN+QKV epilogue layout / attention+proj / MLP)."""
    from mapf_gpt_amd.model import GPT, GPTConfig
    args = weights.model_args(dict(n_layer=1, n_head=5, n_embd=160))
    sd = weights.synthetic_state_dict(args, seed=3, scale=4.0)
    net = GPT(GPTConfig(**args), max_rows=4)
    net.load_state_dict(sd)
    rows = load_tok("mazes000")["tokens"][5, :4]
    tokens = torch.from_numpy(rows).cuda()
    logits = net.logits_tokens(tokens).cpu().numpy()
    ref_logits, layers = gpt_oracle.forward_logits(sd, args, rows, dtype=torch.float64, return_layers=True)
    B, T, C, nh, hs = 4, 256, 160, 5, 32

    def dbg(which, n):
        out = torch.empty(n, dtype=torch.float32, device="cuda")
        _lib.check(_lib.lib().mgpt_gpt_debug_copy(net._h, which, _lib.ptr(out), n, _lib.stream_ptr()))
        return out.cpu().numpy()

    w = {k: torch.as_tensor(v).double() for k, v in sd.items()}
    x0 = layers[0]
    h = torch.nn.functional.layer_norm(x0, (C,), w["transformer.h.0.ln_1.weight"], None, 1e-5)
    qkv = (h @ w["transformer.h.0.attn.c_attn.weight"].t()).view(B, T, 3, nh, hs).permute(2, 0, 3, 1, 4).contiguous()
    got_qkv = dbg(2, 3 * 4 * 256 * C)[: 3 * B * T * C].reshape(3, 4, nh, T, hs)   # planes are max_rows-strided == B here
    assert np.abs(got_qkv - qkv.numpy()).max() < 2e-5, "LN1 + QKV GEMM / head-major scatter"
    x1 = layers[1].numpy()
    got_x = dbg(0, B * T * C).reshape(B, T, C)
    assert np.abs(got_x - x1).max() < 3e-5, "attention / proj / MLP residual stream"
    assert np.abs(logits - ref_logits.numpy()).max() < TOL


def test_forward_chunking_and_row_independence():
    """rows > max_rows are processed in chunks; a row's logits must not depend on its batch neighbours."""
    net = _net("tiny", max_rows=3)
    rows = load_tok("random000")["tokens"][3, :8]
    tokens = torch.from_numpy(rows).cuda()
    full = net.logits_tokens(tokens).cpu().numpy()
    for i in (0, 3, 7):
        one = net.logits_tokens(tokens[i:i + 1]).cpu().numpy()
        assert np.array_equal(one[0], full[i])
    sd = weights.synthetic_state_dict("tiny", seed=0)
    ref = gpt_oracle.forward_logits(sd, weights.model_args("tiny"), rows).numpy()
    assert np.abs(full - ref).max() < TOL


def test_dropout_in_the_config_changes_nothing_at_inference():
    """The reference serves its models in eval mode (inference.py:85), where nn.Dropout is the identity: a checkpoint whose model_args carry
    dropout = 0.1 must give the logits of the same weights with dropout = 0, bit for bit, and stay within 1e-5 of the reference's eval-mode forward."""
    from mapf_gpt_amd.model import GPT, GPTConfig
    rows = load_tok("random000")["tokens"][5, :6]
    tokens = torch.from_numpy(rows).cuda()
    sd = weights.synthetic_state_dict("tiny", seed=0)
    out = {}
    for dp in (0.0, 0.1):
        args = dict(weights.model_args("tiny"), dropout=dp)
        net = GPT(GPTConfig(**args), max_rows=8, precision="f32")
        net.load_state_dict(sd)
        out[dp] = net.logits_tokens(tokens).cpu().numpy()
    assert np.array_equal(out[0.0], out[0.1])
    ref = gpt_oracle.forward_logits(sd, weights.model_args("tiny"), rows).numpy()
    assert np.abs(out[0.1] - ref).max() < TOL


@pytest.mark.envelope_fallback_ok
@pytest.mark.parametrize("name", ["tiny", "2M", "6M"])
def test_bias_true_checkpoint_vs_reference_golden(name):
    """GPTConfig.bias = True (model.py:14-17,29,31,79,81,115; VERDICT r05 "missing" item 4): logits of the real model.py with N(0, 0.02) bias
    vectors on every Linear and LayerNorm (tests/golden/make_golden_bias.py).  The fp32 kernels carry the bias terms; a precision="f16x3"
    request is served by them under the default envelope policy (bit-identical to "f32"), refused under "refuse" / "ignore", and "bf16" is refused."""
    from mapf_gpt_amd.model import GPT, GPTConfig
    g = np.load(os.path.join(GOLDEN, f"gptbias_{name}_s1.npz"))
    plain = np.load(os.path.join(GOLDEN, f"gpt_{name}_s1.npz"))
    assert np.abs(g["logits"] - plain["logits"]).max() > 0.1          # the bias vectors matter: this is not the bias-free golden again
    args = dict(weights.model_args(name), bias=True)
    sd = weights.synthetic_state_dict(args, seed=0, scale=1.0)
    net = GPT(GPTConfig(**args), max_rows=16, precision="f32")
    assert net.load_state_dict(sd) == []
    tokens = torch.from_numpy(g["tokens"]).cuda()
    logits = net.logits_tokens(tokens).cpu().numpy()
    err = np.abs(logits - g["logits"]).max()
    assert err <= TOL, f"{name}: max |dlogit| = {err:.3e}"
    top2 = np.sort(g["logits"][:, :5], axis=1)[:, -2:]
    safe = (top2[:, 1] - top2[:, 0]) > 4 * TOL
    assert np.array_equal(net.act_tokens(tokens, do_sample=False).cpu().numpy()[safe], g["greedy"][safe])
    # the 16-bit kernels have no bias terms: f16x3 falls back (default policy) ...
    assert np.array_equal(net.logits_tokens(tokens, precision="f16x3").cpu().numpy(), logits)
    env = net.envelope()
    assert env["state"] == "outside" and env["effective_precision"] == "f32" and env["probe_err"] is None
    # ... or is refused; bf16 always is
    with pytest.raises(RuntimeError, match="bias"):
        net.logits_tokens(tokens, precision="bf16")
    for policy in ("refuse", "ignore"):
        n2 = GPT(GPTConfig(**args), max_rows=16, precision="f16x3", envelope=policy)
        n2.load_state_dict(sd)
        with pytest.raises(RuntimeError, match="bias"):
            n2.logits_tokens(tokens)
        assert np.array_equal(n2.logits_tokens(tokens, precision="f32").cpu().numpy(), logits)


def test_bias_keys_and_the_config_flag():
    """load_state_dict(strict=False) semantics of the reference (inference.py:83): a bias=False model ignores *.bias keys (unexpected), a bias=True model
    without them keeps its zero-initialised vectors (model.py:152-153) = the bias-free logits; at the C ABI, once one bias tensor is set all are wanted."""
    from mapf_gpt_amd.model import GPT, GPTConfig
    g = np.load(os.path.join(GOLDEN, "gpt_tiny_s1.npz"))
    tokens = torch.from_numpy(g["tokens"]).cuda()
    sd_b = weights.synthetic_state_dict(dict(weights.model_args("tiny"), bias=True), seed=0)
    sd = weights.synthetic_state_dict("tiny", seed=0)
    assert all(np.array_equal(sd[k], sd_b[k]) for k in sd)              # the same weights with and without the flag
    net = GPT(GPTConfig(**weights.model_args("tiny")), max_rows=16)
    unknown = net.load_state_dict(sd_b)
    assert sorted(unknown) == sorted(k for k in sd_b if k.endswith(".bias")) and len(unknown) == 13
    base = net.logits_tokens(tokens).cpu().numpy()
    assert np.abs(base - g["logits"]).max() <= TOL
    assert net.envelope()["state"] in ("undecided", "inside")
    net_b = GPT(GPTConfig(**dict(weights.model_args("tiny"), bias=True)), max_rows=16)
    net_b.load_state_dict(sd)
    assert np.array_equal(net_b.logits_tokens(tokens).cpu().numpy(), base)
    # C ABI: one bias tensor alone -> finalize names what is missing
    h = ctypes.c_void_p()
    L = _lib.lib()
    _lib.check(L.mgpt_gpt_create(ctypes.byref(h), 2, 2, 64, 256, 4))
    for k, v in sd.items():
        a = np.ascontiguousarray(v, dtype=np.float32)
        _lib.check(L.mgpt_gpt_set_param(h, k.encode(), ctypes.c_void_p(a.ctypes.data), a.size, 0))
    a = np.ascontiguousarray(sd_b["transformer.h.1.mlp.c_fc.bias"])
    assert L.mgpt_gpt_set_param(h, b"transformer.h.1.mlp.c_fc.bias", ctypes.c_void_p(a.ctypes.data), a.size - 1, 0) == _lib.ERR_ARG
    _lib.check(L.mgpt_gpt_set_param(h, b"_orig_mod.transformer.h.1.mlp.c_fc.bias", ctypes.c_void_p(a.ctypes.data), a.size, 0))
    assert L.mgpt_gpt_finalize(h) == _lib.ERR_STATE and b"bias tensor #0" in L.mgpt_last_error()
    assert L.mgpt_gpt_set_param(h, b"lm_head.bias", ctypes.c_void_p(a.ctypes.data), 67, 0) == _lib.ERR_ARG     # never exists (model.py:131)
    L.mgpt_gpt_destroy(h)


def _short_cases():
    g = np.load(os.path.join(GOLDEN, "gptshort.npz"))
    keys = sorted({k.rsplit("_", 1)[0] for k in g.files})
    return g, keys


@pytest.mark.parametrize("model", ["tiny_b256", "2M_b256", "6M_b256", "tiny_b100", "85M_b256"])
def test_rows_shorter_than_256_tokens_vs_reference_golden(model):
    """GPT.forward(idx) for idx of T <= block_size tokens (model.py:167-175; VERDICT r05 "missing" item 4): positions 0 .. T-1, attention over the T
    tokens, logits of position T-1 -- goldens from the real model.py (tests/golden/make_golden_short.py), T = 1, ragged lengths, multiples of 32,
    block_size - 1, and a block_size = 100 model.  Served by the exact-fp32 kernels through mgpt_gpt_forward_t."""
    from mapf_gpt_amd.model import GPT, GPTConfig
    g, keys = _short_cases()
    name, block = model.split("_b")
    args = dict(weights.model_args(name), block_size=int(block))
    sd = weights.synthetic_state_dict(args, seed=0, scale=1.0)
    net = GPT(GPTConfig(**args), max_rows=3, precision="f32")          # 4-5 rows through a 3-row workspace: the chunking of the call too
    net.load_state_dict(sd)
    mine = [k for k in keys if k.startswith(model + "_t")]
    assert mine
    for k in mine:
        T = int(k.rsplit("_t", 1)[1])
        idx = torch.from_numpy(g[k + "_tokens"].astype(np.int64)).cuda()
        assert idx.shape[1] == T
        logits, none = net(idx)
        assert none is None and logits.shape == (idx.shape[0], 1, 67)
        err = np.abs(logits[:, 0, :].cpu().numpy() - g[k + "_logits"]).max()
        assert err <= TOL, f"{k}: max |dlogit| = {err:.3e}"
        top2 = np.sort(g[k + "_logits"][:, :5], axis=1)[:, -2:]
        safe = (top2[:, 1] - top2[:, 0]) > 4 * TOL
        assert np.array_equal(net.act(idx, do_sample=False).cpu().numpy()[safe], g[k + "_greedy"][safe])
        drawn = net.act(idx, do_sample=True, generator=torch.Generator(device="cuda").manual_seed(0))
        assert drawn.shape == (idx.shape[0],) and int(drawn.min()) >= 0 and int(drawn.max()) <= 4
    with pytest.raises(ValueError, match="block size is only"):
        net(torch.zeros((1, int(block) + 1), dtype=torch.int64))
    if int(block) == 256:
        # the same kernels with T = 256 as an argument give the 256-token entry point's logits bit for bit
        rows = torch.from_numpy(np.load(os.path.join(GOLDEN, f"gpt_{name}_s1.npz"))["tokens"][:4]).cuda()
        assert torch.equal(net.logits_tokens_t(rows), net.logits_tokens(rows, precision="f32"))
    else:
        with pytest.raises(RuntimeError, match="mgpt_gpt_forward_t"):
            net.logits_tokens(torch.zeros((1, 256), dtype=torch.uint8, device="cuda"))


def test_a_short_row_does_not_see_its_neighbours_or_the_padding():
    """rows * T not a multiple of the GEMMs' 128-token tile: the padding rows of the workspace hold an earlier call's values (here: NaN-producing
    garbage is simulated by a previous call with other tokens); a row's logits depend on its own T tokens only."""
    net = _net("tiny", max_rows=8)
    rows = load_tok("random000")["tokens"][3, :8]
    big = net.logits_tokens(torch.from_numpy(rows).cuda())            # fills the workspaces
    assert torch.isfinite(big).all()
    T = 37
    idx = torch.from_numpy(rows[:, :T].copy()).cuda()
    full = net.logits_tokens_t(idx).cpu().numpy()
    for i in (0, 4, 7):
        assert np.array_equal(net.logits_tokens_t(idx[i:i + 1]).cpu().numpy()[0], full[i])
    sd = weights.synthetic_state_dict("tiny", seed=0)
    ref = gpt_oracle.forward_logits(sd, weights.model_args("tiny"), rows[:, :T]).numpy()
    assert np.abs(full - ref).max() < TOL


def test_device_sampler_matches_host_restatement():
    net = _net("tiny", max_rows=64)
    rows = np.concatenate([load_tok("mazes000")["tokens"][t] for t in range(4)])[:200]
    tokens = torch.from_numpy(rows).cuda()
    logits = torch.empty((200, 67), dtype=torch.float32, device="cuda")
    act = net.act_tokens(tokens, do_sample=True, seed=1234, step=7, logits_out=logits).cpu().numpy()
    exp = np.empty(200, np.int32)
    margin = np.empty(200, np.float32)
    lg = logits.cpu().numpy()
    for r0 in range(0, 200, 64):      # the library keys the RNG by the global row of the call
        e, m = sampling.sample(lg[r0:r0 + 64], 1234, 7, row0=r0)
        exp[r0:r0 + 64], margin[r0:r0 + 64] = e, m
    safe = margin > 1e-5
    assert safe.mean() > 0.99 and np.array_equal(act[safe], exp[safe])
    assert set(np.unique(act)) <= {0, 1, 2, 3, 4}
    a2 = net.act_tokens(tokens, do_sample=True, seed=1234, step=8).cpu().numpy()
    assert (a2 != act).any()          # a different step draws differently


def test_reference_style_act_and_forward_signatures():
    """model.py:167-189 / 244-260 call shapes on the mirror class."""
    net = _net("tiny")
    idx = torch.from_numpy(load_tok("puzzle00")["tokens"][0].astype(np.int64)).cuda()       # LongTensor like inference.py:97
    logits, loss = net(idx)
    assert logits.shape == (4, 1, 67) and loss is None
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    a = net.act(idx, generator=gen)
    assert a.dtype == torch.int64 and a.shape == (4,) and int(a.max()) <= 4
    g = net.act(idx, do_sample=False)
    assert np.array_equal(g.cpu().numpy(), logits[:, 0, :5].argmax(-1).cpu().numpy())
    assert net.act(idx[:1], do_sample=False).dim() == 0           # squeeze() of a single row, model.py:260


@pytest.mark.parametrize("tag", ["tiny_s1", "tiny_s4", "2M_s1", "2M_s4", "6M_s1", "85M_s1"])
def test_f16x3_logits_match_reference_golden(tag):
    """Split-fp16 (3-pass MFMA, fp32 accumulate) path: same 1e-5 bar as the exact fp32 path."""
    from mapf_gpt_amd.model import build_model
    g = np.load(os.path.join(GOLDEN, f"gpt_{tag}.npz"))
    net = build_model(tag.split("_")[0], scale=float(g["scale"]), max_rows=16, precision="f16x3")
    logits = net.logits_tokens(torch.from_numpy(g["tokens"]).cuda()).cpu().numpy()
    err = np.abs(logits - g["logits"]).max()
    assert err <= TOL, f"{tag}: max |dlogit| = {err:.3e}"


@pytest.mark.parametrize("tag", ["tiny_s1", "2M_s1", "2M_s4", "6M_s1"])
def test_bf16_logits_close_to_reference(tag):
    """Single-pass bf16 MFMA mode (the reference's autocast regime, train.py:66-70): bf16-input error class,
    SURVEY.md appendix B measured 4.5e-3 .. 3.5e-2 for torch autocast vs fp64 on these shapes."""
    from mapf_gpt_amd.model import build_model
    g = np.load(os.path.join(GOLDEN, f"gpt_{tag}.npz"))
    net = build_model(tag.split("_")[0], scale=float(g["scale"]), max_rows=16, precision="bf16")
    logits = net.logits_tokens(torch.from_numpy(g["tokens"]).cuda()).cpu().numpy()
    err = np.abs(logits - g["logits"]).max()
    assert err <= 6e-2, f"{tag}: max |dlogit| = {err:.3e}"
    assert err > 1e-6          # it really is the reduced-precision path


@pytest.mark.parametrize("shape,precision", [("2M", "f16x3"), ("6M", "f16x3"), ("6M", "bf16"), ("85M", "bf16"), ("85M", "f16x3")])
def test_chunking_and_batch_position_do_not_change_a_row(shape, precision):
    """Every 16-bit path (fused 2M kernels, pair MLP + packed GEMMs for 6M, packed GEMMs for 85M): ragged chunking
    (max_rows 4, 7 rows -> chunks of 4 + 3) and the position of a row inside the batch leave its logits bit-identical."""
    from mapf_gpt_amd.model import build_model
    rng = np.random.Generator(np.random.PCG64(17))
    tokens = torch.from_numpy(rng.integers(0, 67, (7, 256)).astype(np.uint8)).cuda()
    small = build_model(shape, seed=1, max_rows=4, precision=precision)
    big = build_model(shape, seed=1, max_rows=8, precision=precision)
    a = small.logits_tokens(tokens).cpu().numpy()
    b = big.logits_tokens(tokens).cpu().numpy()
    assert np.array_equal(a, b)
    perm = torch.tensor([6, 2, 5, 0, 3, 1, 4])
    c = big.logits_tokens(tokens[perm].contiguous()).cpu().numpy()
    assert np.array_equal(c, b[perm.numpy()])
    assert np.isfinite(a).all()


@pytest.mark.parametrize("n_head,n_embd,precision,tol", [(4, 256, "f16x3", TOL), (4, 256, "bf16", 6e-2), (8, 512, "f16x3", TOL), (8, 512, "bf16", 6e-2),
                                                      (2, 64, "f16x3", TOL)])
def test_other_shapes_take_the_generic_chain(n_head, n_embd, precision, tol):
    """Shapes that are none of the reference's three (model.py:107-115 allows any): C = 256 with heads of 64 and C = 512 run the
    packed-fragment GEMM chain with the chunk-major residual stream (its bf16 mode with LayerNorm folded into the GEMMs: 2 and 4 partial
    row sums per row), C = 64 the small fused kernels -- logits against the fp64
    torch port of model.py on the same synthetic weights, last-layer shortcut and ragged chunking included (3 rows, max_rows 2)."""
    from mapf_gpt_amd.model import GPT, GPTConfig
    args = weights.model_args(dict(n_layer=2, n_head=n_head, n_embd=n_embd))
    sd = weights.synthetic_state_dict(args, seed=11, scale=2.0)
    net = GPT(GPTConfig(**args), max_rows=2, precision=precision)
    net.load_state_dict(sd)
    rows = load_tok("mazes000")["tokens"][7, :3]
    logits = net.logits_tokens(torch.from_numpy(rows).cuda()).cpu().numpy()
    ref = gpt_oracle.forward_logits(sd, args, rows, dtype=torch.float64).numpy()
    err = np.abs(logits - ref).max()
    assert np.isfinite(logits).all() and err <= tol, f"C={n_embd} heads={n_head} {precision}: max |dlogit| = {err:.3e}"


_ONE_LAYER_REF = {}


def _one_layer_case(n_head, n_embd):
    """(args, state dict, 129 token rows, their fp64 logits) of a one-layer model: computed once per shape, shared by the precisions."""
    if (n_head, n_embd) not in _ONE_LAYER_REF:
        args = weights.model_args(dict(n_layer=1, n_head=n_head, n_embd=n_embd))
        sd = weights.synthetic_state_dict(args, seed=11, scale=2.0)
        rows = np.ascontiguousarray(np.load(os.path.join(GOLDEN, "gptbig_2M_s1.npz"))["tokens"][:129])
        _ONE_LAYER_REF[(n_head, n_embd)] = (args, sd, rows, gpt_oracle.forward_logits(sd, args, rows, dtype=torch.float64).numpy())
    return _ONE_LAYER_REF[(n_head, n_embd)]


@pytest.mark.parametrize("precision,tol", [("f16x3", TOL), ("bf16", 6e-2)])
@pytest.mark.parametrize("n_head,n_embd", [(2, 64), (5, 160), (8, 256)])
def test_one_layer_models_small_and_large_calls(n_head, n_embd, precision, tol):
    """n_layer = 1 of the three fused shapes: layer 0 is also the last layer, so no attention block gathers the embedding or reads the
    (position, token) table, and the whole model is the last-layer launch -- the one-launch tail in a small call (3 rows), attn_last1_kernel
    + the MLP block on the compact rows in a large one (129 rows in one chunk).  Logits against the fp64 torch port of model.py."""
    from mapf_gpt_amd.model import GPT, GPTConfig
    args, sd, rows, ref = _one_layer_case(n_head, n_embd)
    net = GPT(GPTConfig(**args), max_rows=129, precision=precision)
    net.load_state_dict(sd)
    for n in (3, 129):
        logits = net.logits_tokens(torch.from_numpy(np.ascontiguousarray(rows[:n])).cuda()).cpu().numpy()
        err = np.abs(logits - ref[:n]).max()
        print(f"C={n_embd} heads={n_head} {precision} rows={n}: max |dlogit| = {err:.3e}")
        assert np.isfinite(logits).all() and err <= tol, f"C={n_embd} heads={n_head} {precision} rows={n}: max |dlogit| = {err:.3e}"


@pytest.mark.parametrize("name,precision", [("2M", "f16x3"), ("2M", "bf16"), ("tiny", "f16x3"), ("6M", "f16x3"), ("6M", "bf16")])
def test_head_parallel_small_launch_vs_row_per_workgroup_path(name, precision):
    """Round 4: launches of <= 128 rows of the C = 64 / 160 shapes run the attention block head-parallel (one workgroup per
    (row, head), the heads' c_proj contributions folded in head order by the next kernel) -- the way one environment (BASELINE
    cfg1) is served.  The same rows inside a 160-row launch take the row-per-workgroup kernels.  Same products, another
    summation order of the residual stream: the two must agree to fp32 rounding and both must sit within 1e-5 of the fp32 port
    (the f16x3 mode; bf16: its own class).  Round 5: the 6M shape too -- calls of <= 128 rows run attn256_kernel<HP> (one workgroup per
    (row, head), y planes) + the packed-GEMM out-projection instead of the persistent attn256q_kernel (attn256o_kernel until the end of round 5)."""
    from mapf_gpt_amd.model import build_model
    rows = np.load(os.path.join(GOLDEN, "gptbig_2M_s1.npz"))["tokens"][:160]
    net = build_model(name, seed=0, max_rows=160, precision=precision)
    big = net.logits_tokens(torch.from_numpy(rows).cuda()).cpu().numpy()
    for n_small in (1, 40, 128):
        small = net.logits_tokens(torch.from_numpy(np.ascontiguousarray(rows[:n_small])).cuda()).cpu().numpy()
        d = np.abs(small - big[:n_small]).max()
        assert d <= (2e-6 if precision == "f16x3" else 5e-2), f"{name} {precision} {n_small} rows: head-parallel vs fused {d:.3e}"
    # 131 rows: still the row-per-workgroup kernels; the last layer's attn_last1_kernel takes 4 rows per workgroup, the last
    # workgroup here only 3 -- a row's logits do not depend on the launch it is in
    ragged = net.logits_tokens(torch.from_numpy(np.ascontiguousarray(rows[:131])).cuda()).cpu().numpy()
    assert np.array_equal(ragged, big[:131])
    if precision == "f16x3":
        sd, args = weights.synthetic_state_dict(name, seed=0), weights.model_args(name)
        ref = gpt_oracle.forward_logits(sd, args, rows[:40]).numpy()
        assert np.abs(small[:40] - ref).max() <= TOL and np.abs(big[:40] - ref).max() <= TOL


@pytest.mark.parametrize("precision", ["bf16", "f16x3"])
def test_small_call_of_the_packed_gemm_chain_vs_the_large_call(precision):
    """Round 5: a call of <= 128 rows of the packed-GEMM chain (C = 768, the 85M shape) runs its N = 768 GEMMs in 128-row tiles (twice the
    workgroups: 96 tiles of 256 rows leave most CUs idle).  A wave's 64 x 128 sub-tile and its k order do not change, so in the split mode the
    small call reproduces the same rows of a large call BIT FOR BIT.  In the one-plane mode a large call runs the GEMMs on the 16 x 16 x 32
    MFMA (gemm_pk16_kernel; a small call is not power-limited and keeps the 32 x 32 x 16 kernel): another summation order inside the MFMA,
    so the two agree to the mode's own class -- and two LARGE calls of different sizes (160 rows in one launch, 200 rows through chunks of
    160 + 40) agree bit for bit: the kernels are chosen per call, not per chunk."""
    from mapf_gpt_amd.model import build_model
    rows = np.load(os.path.join(GOLDEN, "gptbig_2M_s1.npz"))["tokens"][:200]
    net = build_model("85M", seed=0, max_rows=160, precision=precision)
    big = net.logits_tokens(torch.from_numpy(np.ascontiguousarray(rows[:160])).cuda()).cpu().numpy()
    assert np.isfinite(big).all()
    for n_small in (1, 32, 128):
        small = net.logits_tokens(torch.from_numpy(np.ascontiguousarray(rows[:n_small])).cuda()).cpu().numpy()
        d = np.abs(small - big[:n_small]).max()
        if precision == "f16x3":
            assert np.array_equal(small, big[:n_small]), f"85M f16x3, {n_small} rows: {d:.3e}"
        else:
            assert d <= 5e-2, f"85M bf16, {n_small} rows: small vs large call {d:.3e}"
    chunked = net.logits_tokens(torch.from_numpy(rows).cuda()).cpu().numpy()          # 200 rows: chunks of 160 + 40, a LARGE call
    assert np.array_equal(chunked[:160], big), "a row's logits depend on the large call it is in"


@pytest.mark.parametrize("name,precision", [("2M", "f16x3"), ("6M", "f16x3"), ("6M", "bf16")])
def test_persistent_kernels_uneven_grid(name, precision):
    """The persistent attention kernels (attn256q_kernel, attn160o_kernel; grid = min(rows, CUs), a workgroup walks rows b, b + grid, ...)
    with a row count that is not a multiple of the grid: 600 rows on 256 CUs = 88 workgroups take 3 rows, 168 take 2, and the last
    layer's attn_last1_kernel handles 150 workgroups of 4.  A row's logits are bit-identical to the same row in a 200-row launch (one
    row per workgroup) and, in the 1e-5 mode, within the bar of the reference goldens."""
    from mapf_gpt_amd.model import build_model
    g = np.load(os.path.join(GOLDEN, f"gptbig_{name}_s1.npz"))
    base = g["tokens"]                                                   # 256 distinct rows
    rows = np.ascontiguousarray(np.concatenate([base, base[::-1], base[:88]]))        # 600 rows
    net = build_model(name, seed=0, max_rows=600, precision=precision)
    big = net.logits_tokens(torch.from_numpy(rows).cuda()).cpu().numpy()
    small = net.logits_tokens(torch.from_numpy(np.ascontiguousarray(rows[:200])).cuda()).cpu().numpy()
    assert np.array_equal(big[:200], small)
    assert np.array_equal(big[256:512], big[:256][::-1]) and np.array_equal(big[512:], big[:88])
    if precision == "f16x3":
        assert np.abs(big[:256] - g["logits_f32"]).max() <= TOL


def test_spread_scores_take_the_exact_attention_loop():
    """Round 5: the 6M attention kernel's key-tile loop takes ONE softmax reference per query and head (the maximum of the first key
    tile) and falls back to the exact running-maximum loop when exp2(s - ref) leaves the fp16 range of the P planes
    (gpt_kernels_attn_tiles.h).  N(0, 0.02) weights never get there (counter 0, and the goldens above pin that path); here the q and k
    rows of c_attn are scaled until scores spread by tens of nats, so that a good share of the (wave, head) pairs must fall back.
    Both paths together must stay in the f16x3 class against our exact-fp32-MFMA path (whose attention is a different kernel)."""
    from mapf_gpt_amd.model import build_model
    rng = np.random.Generator(np.random.PCG64(23))
    tok = torch.from_numpy(np.load(os.path.join(GOLDEN, "gptbig_6M_s1.npz"))["tokens"][:160]).cuda()   # (> 128 rows: the persistent kernels)
    _lib.debug_counter(0, reset=True)
    net = build_model("6M", seed=0, max_rows=160, precision="f16x3")
    plain = net.logits_tokens(tok).cpu().numpy()
    assert _lib.debug_counter(0, reset=True) == 0, "synthetic N(0, 0.02) weights must stay on the pipelined loop"
    sd = weights.synthetic_state_dict("6M", seed=0)
    for layer in (1, 2, 4):
        w = sd[f"transformer.h.{layer}.attn.c_attn.weight"]
        w[:512] *= 7.0                                     # q and k rows: scores x 49
    a = build_model("6M", precision="f32", max_rows=160, state_dict=sd).logits_tokens(tok).cpu().numpy()
    _lib.debug_counter(0, reset=True)
    b = build_model("6M", precision="f16x3", max_rows=160, state_dict=sd, envelope="ignore").logits_tokens(tok).cpu().numpy()   # (rms 0.115: outside the envelope)
    n_fallback = _lib.debug_counter(0, reset=True)
    err = float(np.abs(a - b).max())
    print(f"spread scores: {n_fallback} (wave, head) fallbacks of {160 * 8 * 8 * 7}, max |f16x3 - f32| = {err:.3e}, |logits| <= {np.abs(a).max():.2f}")
    assert n_fallback > 0, "the scaled checkpoint was meant to leave the fp16 range of the P planes somewhere"
    assert np.isfinite(b).all() and err <= 3e-5, f"max |f16x3 - f32| = {err:.3e}"
    assert np.abs(plain - a).max() > 1e-3                  # (the scaling really changed the function)


@pytest.mark.parametrize("name,precision", [("2M", "f16x3"), ("2M", "bf16"), ("tiny", "f16x3")])
def test_remainder_chunk_of_a_large_call_keeps_the_large_launch_kernels(name, precision):
    """the head-parallel small-launch kernels (<= 128 rows) sum the residual stream in another order than the
    row-per-workgroup kernels, so the choice between them must be a property of the CALL, not of the chunk a row happens to fall
    into.  200 rows through a context of max_rows 128 (chunks of 128 + 72) and through one of max_rows 256 (one launch) must agree
    bit for bit -- the 72-row remainder stays on the large-launch kernels -- and so must mgpt_gpt_act's own chunking."""
    from mapf_gpt_amd.model import build_model
    rows = np.ascontiguousarray(np.load(os.path.join(GOLDEN, "gptbig_2M_s1.npz"))["tokens"][:200])
    tok = torch.from_numpy(rows).cuda()
    a = build_model(name, seed=0, max_rows=128, precision=precision)
    b = build_model(name, seed=0, max_rows=256, precision=precision)
    la, lb = a.logits_tokens(tok).cpu().numpy(), b.logits_tokens(tok).cpu().numpy()
    assert np.array_equal(la, lb)
    assert torch.equal(a.act_tokens(tok, do_sample=False), b.act_tokens(tok, do_sample=False))
