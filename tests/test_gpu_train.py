"""Training on the device (GPT.forward_backward, clip_grad_norm_, configure_optimizers -> AdamW; include/mapf_gpt_amd.h mgpt_gpt_train_*):
gradients against fp64 autograd of the pinned oracle's restatement of model.py, loss, determinism, accumulation, chunking, clip + AdamW
against torch's, optimizer state round trip, inference after training in every precision, and a short training run on expert rows."""
import functools

import numpy as np
import pytest
import torch

from mapf_gpt_amd import _lib, weights
from mapf_gpt_amd.model import GPT, GPTConfig, build_model
from tests.train_ref import LOCALISERS, expert_rows, leaves, loss_and_grads, targets_last, targets_mixed, trained_like_case

pytestmark = pytest.mark.gpu


def _rows(n, seed=0):
    return expert_rows(n, seed)


def _targets(case, tokens, actions, seed=1):
    rows = len(tokens)
    if case == "last":
        return targets_last(actions)
    if case == "mixed":
        return targets_mixed(rows, seed)
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 67, (rows, 256)).astype(np.int64)


def _net(name, max_rows=4, seed=0, train_rows=None):
    net = build_model(name, seed=seed, max_rows=max_rows)
    net._sd = weights.synthetic_state_dict(name, seed=seed)
    net._args = weights.model_args(name)
    return net.train(max_rows=train_rows)


def _dev_grads(net):
    return {k: v.double().cpu() for k, v in net.grads().items()}


def _grad_figures(got, g64, g32):
    """per tensor: (name, max|g - g64|, the bar max(4 x fp32-autograd error, 1e-6 max|g64|), fp32-autograd error, max|g64|)"""
    out = []
    for k, ref in g64.items():
        m = float(ref.abs().max())
        err = float((got[k] - ref).abs().max())
        e32 = float((g32[k].double() - ref).abs().max())
        out.append((k, err, max(4 * e32, 1e-6 * m), e32, m))
    return out


def _check_grads(name, got, g64, g32):
    figures = _grad_figures(got, g64, g32)
    k, err, bar, _, _ = max(figures, key=lambda f: f[1] / max(f[2], 1e-300))
    print(f"{name}: worst error / bar {err / max(bar, 1e-300):.3f} ({k})")
    worst = 0.0
    for k, err, bar, e32, m in figures:
        assert np.isfinite(err), f"{name} {k}: gradient not finite"
        assert err <= bar and err <= 1e-4 * m, f"{name} {k}: max|g - g64| {err:.3e}, bar {bar:.3e} (fp32 autograd {e32:.3e}, max|g64| {m:.3e})"
        worst = max(worst, err / max(m, 1e-30))
    return worst


@pytest.mark.parametrize("name", ["tiny", "2M", "6M", "85M"])
@pytest.mark.parametrize("case", ["last", "all", "mixed"])
def test_gradients_match_fp64_autograd(case, name):
    rows = 2 if name == "85M" else 3
    tokens, actions = _rows(rows, seed=len(name))
    targets = _targets(case, tokens, actions)
    net = _net(name)
    net.zero_grad()
    loss = float(net.forward_backward(torch.as_tensor(tokens), torch.as_tensor(targets)))
    got = _dev_grads(net)
    l64, g64 = loss_and_grads(net._sd, net._args, tokens, targets, torch.float64)
    _, g32 = loss_and_grads(net._sd, net._args, tokens, targets, torch.float32)
    assert set(got) == set(g64)
    _check_grads(f"{name}/{case}", got, g64, g32)
    assert abs(loss - l64) <= 1e-5 * abs(l64), (loss, l64)
    # the loss equals the f32 sequence forward's (the same kernels up to the head)
    _, lf = net.forward(torch.as_tensor(tokens).cuda(), torch.as_tensor(targets).cuda())
    assert abs(loss - float(lf)) <= 1e-6 * abs(float(lf)), (loss, float(lf))


def test_deterministic_and_accumulating():
    tokens, actions = _rows(4, seed=3)
    targets = _targets("mixed", tokens, actions)
    net = _net("6M")
    net.zero_grad()
    net.forward_backward(torch.as_tensor(tokens), torch.as_tensor(targets))
    a = _dev_grads(net)
    net.zero_grad()
    net.forward_backward(torch.as_tensor(tokens), torch.as_tensor(targets))
    b = _dev_grads(net)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k}: two identical calls differ"
    # two micro-steps with loss_scale 0.5 (train.py:324-331, gradient_accumulation_steps = 2) against the restatement's
    net.zero_grad()
    t1, a1 = tokens[:2], targets[:2]
    t2, a2 = tokens[2:], _targets("last", tokens[2:], actions[2:])
    net.forward_backward(torch.as_tensor(t1), torch.as_tensor(a1), loss_scale=0.5)
    net.forward_backward(torch.as_tensor(t2), torch.as_tensor(a2), loss_scale=0.5)
    got = _dev_grads(net)
    _, g64 = loss_and_grads(net._sd, net._args, None, None, torch.float64, 0.5, micro=[(t1, a1), (t2, a2)])
    _, g32 = loss_and_grads(net._sd, net._args, None, None, torch.float32, 0.5, micro=[(t1, a1), (t2, a2)])
    _check_grads("accumulation", got, g64, g32)


def test_chunked_call_matches_one_chunk():
    tokens, actions = _rows(5, seed=4)
    targets = _targets("mixed", tokens, actions)
    small = _net("tiny", train_rows=2)             # 5 rows in chunks of 2, 2, 1: one normaliser for the whole call
    small.zero_grad()
    ls = float(small.forward_backward(torch.as_tensor(tokens), torch.as_tensor(targets)))
    l64, g64 = loss_and_grads(small._sd, small._args, tokens, targets, torch.float64)
    _, g32 = loss_and_grads(small._sd, small._args, tokens, targets, torch.float32)
    _check_grads("chunked", _dev_grads(small), g64, g32)
    assert abs(ls - l64) <= 1e-5 * l64


# ----- the trained-like regime (tests/train_ref.py: trained_like_state_dict; tests/test_train_cpu.py pins it): peaked attention, GELU tails,
# LayerNorm gains of both signs.  At N(0, 0.02) attention is nearly uniform and a key or slot mix-up changes a ~10 % correction only.
def _trained_net(args, sd, max_rows=4, train_rows=None):
    net = build_model(args, state_dict=sd, max_rows=max_rows)
    net._sd, net._args = sd, args
    return net.train(max_rows=train_rows)


@functools.lru_cache(maxsize=None)
def _trained_ref(name, rows=None):
    """one fp64 and one fp32 autograd run per case, shared by the tests that need it and left unchanged"""
    tokens, targets, sd, args = trained_like_case(name, rows)
    l64, g64 = loss_and_grads(sd, args, tokens, targets, torch.float64)
    _, g32 = loss_and_grads(sd, args, tokens, targets, torch.float32)
    return tokens, targets, sd, args, l64, g64, g32


def _by_kernel(g, C):
    """the block gradients of a one-layer model, c_attn.weight's by its q, k and v thirds: a failure names a kernel"""
    p = "transformer.h.0."
    out = {f"c_attn.{nm}": g[p + "attn.c_attn.weight"][i * C:(i + 1) * C] for i, nm in enumerate("qkv")}
    out.update({nm: g[p + nm + ".weight"] for nm in ("attn.c_proj", "ln_1", "ln_2", "mlp.c_fc", "mlp.c_proj")})
    return out


def _kernel_report(name, got, g64, g32, C):
    figures = _grad_figures(*(_by_kernel(g, C) for g in (got, g64, g32)))
    return f"{name} by kernel: " + "; ".join(f"{k} {err:.3e} = {err / max(bar, 1e-300):.2f} x bar (max|g64| {m:.3e})" for k, err, bar, _, m in figures)


@pytest.mark.parametrize("name", ["tiny", "2M", "6M", "85M", *LOCALISERS])
def test_trained_like_gradients_match_fp64_autograd(name):
    tokens, targets, sd, args, l64, g64, g32 = _trained_ref(name)
    net = _trained_net(args, sd)
    tk, tg = torch.as_tensor(tokens), torch.as_tensor(targets)
    net.zero_grad()
    loss = float(net.forward_backward(tk, tg))
    got = _dev_grads(net)
    assert set(got) == set(g64)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), f"{name} {k}: gradient not finite"
    try:
        _check_grads(f"trained-like {name}", got, g64, g32)
    except AssertionError as e:
        if name in LOCALISERS:
            raise AssertionError(f"{e}\n{_kernel_report(name, got, g64, g32, args['n_embd'])}") from None
        raise
    assert abs(loss - l64) <= 1e-5 * abs(l64), (loss, l64)
    net.zero_grad()
    again = float(net.forward_backward(tk, tg))
    b = _dev_grads(net)
    assert again == loss
    for k in got:
        assert torch.equal(got[k], b[k]), f"{name} {k}: two identical calls differ"


# ----- ragged and empty weight-gradient slabs (train.hip: slabs_of, slab_tokens, kMaxSlabs = 64).  Up to 64 rows a slab is 256 tokens and
# every slab is full.  65 rows: 16640 tokens in 64 slabs of 272 (fp32; slab 61 holds 48 tokens, 62 and 63 none) or of 288 (bf16; slab 57
# holds 224, 58 - 63 none).  130 rows: slabs of 528 (fp32; slab 63 holds 16) or 544 (bf16; slab 61 holds 96, 62 and 63 none).
@pytest.mark.parametrize("rows", [65, 130])
def test_ragged_weight_gradient_slabs(rows):
    tokens, targets, sd, args, l64, g64, g32 = _trained_ref("tiny", rows)
    net = _trained_net(args, sd, train_rows=rows)
    net.zero_grad()
    loss = float(net.forward_backward(torch.as_tensor(tokens), torch.as_tensor(targets)))
    _check_grads(f"{rows} rows, one chunk", _dev_grads(net), g64, g32)
    assert abs(loss - l64) <= 1e-5 * abs(l64), (loss, l64)
    if rows == 130:
        # ... and as two full chunks of 65 rows: the same bars, the same loss
        net.train(max_rows=65)
        net.zero_grad()
        two = float(net.forward_backward(torch.as_tensor(tokens), torch.as_tensor(targets)))
        _check_grads("130 rows, chunks of 65", _dev_grads(net), g64, g32)
        assert abs(two - l64) <= 1e-5 * abs(l64), (two, l64)
        assert abs(two - loss) <= 1e-6 * abs(loss), (two, loss)


def test_one_targeted_position():
    """count = 1: the call's normaliser is 1, every other token's dlogits row is zero"""
    tokens, _, sd, args = trained_like_case("tiny", 2)
    targets = np.full((2, 256), -1, np.int64)
    targets[1, 137] = 41
    net = _trained_net(args, sd)
    net.zero_grad()
    loss = float(net.forward_backward(torch.as_tensor(tokens), torch.as_tensor(targets)))
    l64, g64 = loss_and_grads(sd, args, tokens, targets, torch.float64)
    _, g32 = loss_and_grads(sd, args, tokens, targets, torch.float32)
    _check_grads("one target", _dev_grads(net), g64, g32)
    assert abs(loss - l64) <= 1e-5 * abs(l64), (loss, l64)


def test_refusals():
    net = _net("tiny")
    tokens, _ = _rows(2)
    with pytest.raises(_lib.MGPTError) as e:                 # no targeted position: torch would return NaN
        net.forward_backward(torch.as_tensor(tokens), torch.full((2, 256), -1))
    assert e.value.code == _lib.ERR_ARG
    with pytest.raises(_lib.MGPTError) as e:
        net.forward_backward(torch.as_tensor(tokens), torch.full((2, 256), 67))
    assert e.value.code == _lib.ERR_ARG
    with pytest.raises(_lib.MGPTError) as e:                 # T != 256
        net.forward_backward(torch.as_tensor(tokens[:, :128]), torch.zeros((2, 128), dtype=torch.int64))
    assert e.value.code == _lib.ERR_ARG
    a = weights.model_args("tiny")
    a["bias"] = True
    nb = GPT(GPTConfig(**a), max_rows=2)
    nb.load_state_dict(weights.synthetic_state_dict(a, seed=0))
    with pytest.raises(_lib.MGPTError) as e:
        nb.train()
    assert e.value.code == _lib.ERR_UNSUPPORTED
    a = weights.model_args("tiny")
    a["dropout"] = 0.1
    nd = GPT(GPTConfig(**a), max_rows=2)
    nd.load_state_dict(weights.synthetic_state_dict("tiny", seed=0))
    with pytest.raises(NotImplementedError):
        nd.train()


def _torch_adamw(sd, names_shapes, wd, lr, betas):
    lv, _ = leaves(sd, torch.float64)
    decay = [lv[n] for n, s in names_shapes if len(s) >= 2]
    nodecay = [lv[n] for n, s in names_shapes if len(s) < 2]
    opt = torch.optim.AdamW([{"params": decay, "weight_decay": wd}, {"params": nodecay, "weight_decay": 0.0}], lr=lr, betas=betas)
    return lv, opt


def test_clip_and_adamw_match_torch():
    tokens, actions = _rows(4, seed=5)
    net = _net("tiny")
    opt = net.configure_optimizers(0.1, 6e-4, (0.9, 0.95), "cuda")
    lv, topt = _torch_adamw(net._sd, net.named_parameters(), 0.1, 6e-4, (0.9, 0.95))
    for it in range(3):
        net.zero_grad()
        net.forward_backward(torch.as_tensor(tokens[:2]), torch.as_tensor(targets_last(actions[:2])), loss_scale=0.5)
        net.forward_backward(torch.as_tensor(tokens[2:]), torch.as_tensor(_targets("all", tokens[2:], actions[2:], seed=it)), loss_scale=0.5)
        g = _dev_grads(net)                                  # the library's own gradients into torch's clip + AdamW (fp64)
        for n, v in lv.items():
            v.grad = g[n].clone()
        tn = float(torch.nn.utils.clip_grad_norm_(list(lv.values()), 1.0))
        total = float(net.clip_grad_norm_(1.0))
        assert abs(total - tn) <= 1e-6 * tn + 1e-9, (total, tn)
        gc = _dev_grads(net)
        for n, v in lv.items():
            assert float((gc[n] - v.grad).abs().max()) <= 1e-6 * float(v.grad.abs().max()) + 1e-12, n
        opt.step()
        topt.step()
        sd = net.state_dict()
        for n, v in lv.items():
            d = float((sd[n].double().cpu() - v.detach()).abs().max())
            assert d <= 1e-6 * float(v.detach().abs().max()) + 1e-9, (it, n, d)
        # torch keeps the parameters on their own track from here: feed ours back so that only one step's rounding is compared
        with torch.no_grad():
            for n, v in lv.items():
                v.copy_(sd[n].double().cpu())
    # optimizer state: torch.optim.AdamW.state_dict() layout, loads into torch and continues the same way
    osd = opt.state_dict()
    assert [len(gp["params"]) for gp in osd["param_groups"]] == [len(gp["params"]) for gp in topt.state_dict()["param_groups"]]
    t2 = torch.optim.AdamW([{"params": [v for n, v in lv.items() if v.dim() >= 2], "weight_decay": 0.1},
                            {"params": [v for n, v in lv.items() if v.dim() < 2], "weight_decay": 0.0}], lr=6e-4, betas=(0.9, 0.95))
    cpu_osd = {"state": {i: {k: (t.double().cpu() if k != "step" else t) for k, t in s.items()} for i, s in osd["state"].items()},
               "param_groups": osd["param_groups"]}
    t2.load_state_dict(cpu_osd)
    for i, st in t2.state_dict()["state"].items():
        assert float(st["step"]) == 3.0
    # ... and continues the same way: one more step of both on the library's clipped gradients
    net.zero_grad()
    net.forward_backward(torch.as_tensor(tokens), torch.as_tensor(_targets("mixed", tokens, actions, seed=9)))
    net.clip_grad_norm_(1.0)
    g = _dev_grads(net)
    for n, v in lv.items():
        v.grad = g[n].clone()
    opt.step()
    t2.step()
    sd = net.state_dict()
    for n, v in lv.items():
        d = float((sd[n].double().cpu() - v.detach()).abs().max())
        assert d <= 1e-6 * float(v.detach().abs().max()) + 1e-9, (n, d)
    # and back: a fresh model loaded from state_dict() and the optimizer state continues bit for bit with the original
    net2 = build_model("tiny", state_dict={k: v.cpu() for k, v in net.state_dict().items()}, max_rows=4).train()
    opt2 = net2.configure_optimizers(0.1, 6e-4, (0.9, 0.95), "cuda")
    opt2.load_state_dict(opt.state_dict())
    for m, o in ((net, opt), (net2, opt2)):
        m.zero_grad()
        m.forward_backward(torch.as_tensor(tokens), torch.as_tensor(targets_last(actions)))
        m.clip_grad_norm_(1.0)
        o.step()
    s1, s2 = net.state_dict(), net2.state_dict()
    for k in s1:
        assert torch.equal(s1[k], s2[k]), k


def test_clip_above_the_total_norm_changes_nothing():
    tokens, targets, sd, args, *_ = _trained_ref("tiny")
    net = _trained_net(args, sd)
    net.zero_grad()
    net.forward_backward(torch.as_tensor(tokens), torch.as_tensor(targets))
    before = _dev_grads(net)
    lv, _ = leaves(sd, torch.float64)
    for n, v in lv.items():
        v.grad = before[n].clone()
    tn = float(torch.nn.utils.clip_grad_norm_(list(lv.values()), 1e30))
    total = float(net.clip_grad_norm_(2.0 * tn))              # coefficient min(2 tn / (tn + 1e-6), 1) = 1
    assert abs(total - tn) <= 1e-6 * tn, (total, tn)
    after = _dev_grads(net)
    for k in before:
        assert torch.equal(before[k], after[k]), f"{k}: a clip above the total norm changed the gradient"


def test_clip_and_adamw_on_the_trained_like_checkpoint():
    """one clip + AdamW step where the total norm is far above max_norm (about 30 on this checkpoint: a coefficient near 0.03)"""
    tokens, targets, sd, args, *_ = _trained_ref("2M")
    net = _trained_net(args, sd)
    opt = net.configure_optimizers(0.1, 6e-4, (0.9, 0.95), "cuda")
    lv, topt = _torch_adamw(sd, net.named_parameters(), 0.1, 6e-4, (0.9, 0.95))
    net.zero_grad()
    net.forward_backward(torch.as_tensor(tokens), torch.as_tensor(targets))
    g = _dev_grads(net)                                       # the library's own gradients into torch's clip + AdamW (fp64)
    for n, v in lv.items():
        v.grad = g[n].clone()
    tn = float(torch.nn.utils.clip_grad_norm_(list(lv.values()), 1.0))
    assert tn > 10.0, tn
    total = float(net.clip_grad_norm_(1.0))
    assert abs(total - tn) <= 1e-6 * tn + 1e-9, (total, tn)
    gc = _dev_grads(net)
    for n, v in lv.items():
        assert float((gc[n] - v.grad).abs().max()) <= 1e-6 * float(v.grad.abs().max()) + 1e-12, n
    opt.step()
    topt.step()
    new = net.state_dict()
    for n, v in lv.items():
        d = float((new[n].double().cpu() - v.detach()).abs().max())
        assert d <= 1e-6 * float(v.detach().abs().max()) + 1e-9, (n, d)


def test_inference_after_training_serves_new_weights():
    from mapf_gpt_amd import maps
    from mapf_gpt_amd.runner import BatchedRunner, make_instances
    tokens, actions = _rows(8, seed=6)
    net = _net("6M", max_rows=64)
    grid, s_ok, g_ok = maps.load_named("validation-random-seed-000")
    pos, goal = make_instances(grid, 2, 8, 0, s_ok, g_ok)
    run = BatchedRunner(grid, 2, 8, net, max_episode_steps=16, seed=1, do_sample=False, precision="f16x3")
    run.reset(pos, goal)
    for _ in range(3):
        run.step()                                    # eager, then a captured graph
    tok_dev = torch.as_tensor(tokens).to(torch.uint8).cuda()
    before = {p: net.logits_tokens(tok_dev, precision=p).clone() for p in ("f32", "f16x3", "bf16")}
    opt = net.configure_optimizers(0.1, 1e-3, (0.9, 0.95))
    for _ in range(2):
        net.zero_grad()
        net.forward_backward(torch.as_tensor(tokens), torch.as_tensor(targets_last(actions)))
        net.clip_grad_norm_(1.0)
        opt.step()
    fresh = build_model("6M", state_dict={k: v.cpu() for k, v in net.state_dict().items()}, max_rows=64)
    for p in ("f32", "f16x3", "bf16"):
        got, ref = net.logits_tokens(tok_dev, precision=p), fresh.logits_tokens(tok_dev, precision=p)
        assert torch.equal(got, ref), p
        assert not torch.equal(got, before[p]), p
        assert torch.equal(net.act_tokens(tok_dev, do_sample=False, precision=p), fresh.act_tokens(tok_dev, do_sample=False, precision=p)), p
    # the graph captured before the step re-captures: the runner's next step serves the new weights (tokens of this step through `fresh`)
    run.step()
    acts = run.actions.view(-1).clone()
    ref = fresh.act_tokens(run.tokens, do_sample=False, precision="f16x3")
    assert torch.equal(acts.to(ref.dtype), ref)


def test_tiny_learns_expert_rows():
    tokens, actions = _rows(388, seed=7)
    net = _net("tiny", max_rows=64)
    # (lr 1.5e-3: stable for 20 iterations; at 3e-3 a loss spike near iteration 14 amplifies fp32 rounding between the two runs)
    opt = net.configure_optimizers(0.1, 1.5e-3, (0.9, 0.95))
    lv32, _ = leaves(net._sd, torch.float32)
    decay = [lv32[n] for n, s in net.named_parameters() if len(s) >= 2]
    nodecay = [lv32[n] for n, s in net.named_parameters() if len(s) < 2]
    topt = torch.optim.AdamW([{"params": decay, "weight_decay": 0.1}, {"params": nodecay, "weight_decay": 0.0}], lr=1.5e-3, betas=(0.9, 0.95))
    from tests.test_loss_cpu import seq_oracle
    ours, theirs = [], []
    for it in range(20):
        sel = np.random.Generator(np.random.PCG64(it)).integers(0, len(tokens), 32)
        x, y = tokens[sel], targets_last(actions[sel])
        net.zero_grad()
        ours.append(float(net.forward_backward(torch.as_tensor(x), torch.as_tensor(y))))
        net.clip_grad_norm_(1.0)
        opt.step()
        topt.zero_grad()
        view = dict(lv32)
        view["lm_head.weight"] = lv32["transformer.wte.weight"]
        _, loss = seq_oracle(view, net._args, x, torch.as_tensor(y), dtype=torch.float32)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(lv32.values()), 1.0)
        topt.step()
        theirs.append(float(loss))
    ours, theirs = np.array(ours), np.array(theirs)
    rel = np.abs(ours - theirs) / theirs
    assert rel[:5].max() <= 1e-3 and rel.max() <= 1e-2, (ours, theirs)
    assert ours[-3:].mean() < 0.8 * ours[0], ours          # from ln(67) ~ 4.2 towards the 5 actions' prior


def test_train_again_keeps_the_optimizer_state():
    """train.py calls model.eval() / model.train() around every evaluation (train.py:246,258,293,295): the workspace, the gradients and the
    AdamW state survive; a re-size (train(max_rows=k)) keeps them too."""
    tokens, actions = _rows(4, seed=8)
    net = _net("tiny", train_rows=4)
    opt = net.configure_optimizers(0.1, 6e-4, (0.9, 0.95))
    net.zero_grad()
    net.forward_backward(torch.as_tensor(tokens), torch.as_tensor(targets_last(actions)))
    net.clip_grad_norm_(1.0)
    opt.step()
    net.forward_backward(torch.as_tensor(tokens), torch.as_tensor(_targets("all", tokens, actions)))     # gradients left non-zero

    def snap():
        st = {i: {k: v.detach().cpu().clone() for k, v in s.items()} for i, s in opt.state_dict()["state"].items()}
        return st, {k: v.cpu() for k, v in net.grads().items()}

    def same(a, b):
        assert a[0].keys() == b[0].keys() and a[1].keys() == b[1].keys()
        for i in a[0]:
            for k in a[0][i]:
                assert torch.equal(a[0][i][k], b[0][i][k]), (i, k)
        for k in a[1]:
            assert torch.equal(a[1][k], b[1][k]), k

    s0 = snap()
    assert len(s0[0]) == len(net.named_parameters()) and all(float(v["step"]) == 1.0 for v in s0[0].values())
    net.eval()
    net.train()
    same(s0, snap())
    net.train(max_rows=2)                         # re-size: activations only
    same(s0, snap())
    # the re-sized workspace trains (4 rows in chunks of 2) and continues from the kept state
    net.zero_grad()
    loss = float(net.forward_backward(torch.as_tensor(tokens), torch.as_tensor(targets_last(actions))))
    l64, g64 = loss_and_grads({k: v.cpu().numpy() for k, v in net.state_dict().items()}, net._args, tokens, targets_last(actions))
    assert abs(loss - l64) <= 1e-5 * l64
    opt.step()
    assert all(float(v["step"]) == 2.0 for v in opt.state_dict()["state"].values())


def test_state_dict_needs_no_training_workspace():
    net = build_model("tiny", seed=3, max_rows=2)
    sd = net.state_dict()
    ref = weights.synthetic_state_dict("tiny", seed=3)
    assert set(sd) == set(ref)
    for k in ref:
        assert np.array_equal(sd[k].cpu().numpy(), ref[k]), k
    assert getattr(net, "_train_rows", None) is None and not net.training
    a = weights.model_args("tiny")
    a["dropout"] = 0.1                            # an inference-only model (dropout is the identity there) reads back too
    nd = GPT(GPTConfig(**a), max_rows=2)
    nd.load_state_dict(ref)
    assert torch.equal(nd.state_dict()["transformer.wte.weight"].cpu(), torch.from_numpy(ref["transformer.wte.weight"]))


def test_training_cli_writes_a_loadable_checkpoint_and_resumes(tmp_path):
    import json
    import subprocess
    import sys
    pa = pytest.importorskip("pyarrow")
    from mapf_gpt_amd.inference import MAPFGPTInference, MAPFGPTInferenceConfig
    from tests.helpers import ROOT
    x, y = _rows(96, seed=9)
    shard = tmp_path / "train.arrow"
    table = pa.table({"input_tensors": pa.array(list(x.astype(np.int8))), "gt_actions": pa.array(y.astype(np.int8))})
    with pa.OSFile(str(shard), "wb") as sink:
        with pa.ipc.new_file(sink, table.schema) as w:
            w.write_table(table)
    out = tmp_path / "out"
    common = ["--data", str(shard), "--val", str(shard), "--out-dir", str(out), "--eval-interval", "2", "--eval-iters", "2",
              "--batch-size", "16", "--gradient-accumulation-steps", "2", "--warmup-iters", "2", "--lr-decay-iters", "6",
              "--learning-rate", "1e-3", "--min-lr", "1e-4"]

    def run(*extra):
        r = subprocess.run([sys.executable, "-m", "mapf_gpt_amd.training", *extra, *common], cwd=ROOT, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]

    lines = run("--init", "tiny", "--max-iters", "4")
    evals = [l for l in lines if "val_loss" in l]
    assert [e["iter"] for e in evals] == [0, 2, 4] and lines[-1]["iter"] == 5
    assert all(np.isfinite(e["val_loss"]) and np.isfinite(e["train_loss"]) for e in evals)
    assert evals[0]["lr"] == 0.0 and abs(evals[1]["lr"] - 1e-3) < 1e-12      # warmup: lr(0) = 0, lr(2) = learning_rate
    ck = out / "ckpt.pt"
    raw = torch.load(ck, map_location="cpu", weights_only=True)
    assert set(raw) == {"model", "optimizer", "model_args", "iter_num", "best_val_loss", "config"} and raw["iter_num"] == 4
    assert all(float(s["step"]) == 4.0 for s in raw["optimizer"]["state"].values())
    args, sd = weights.load_checkpoint(str(ck))
    assert (args["n_layer"], args["n_embd"]) == (2, 64)
    algo = MAPFGPTInference(MAPFGPTInferenceConfig(path_to_weights=str(ck), device="cuda"))
    got = algo.net.state_dict()
    for k in sd:
        assert np.array_equal(got[k].cpu().numpy(), sd[k]), k
    # resume (train.py:190-226): optimizer state, iter_num and best_val_loss come back; the step counts continue
    lines = run("--init", str(ck), "--resume", "--max-iters", "6")
    evals = [l for l in lines if "val_loss" in l]
    assert [e["iter"] for e in evals] == [4, 6] and lines[-1]["iter"] == 7
    raw = torch.load(ck, map_location="cpu", weights_only=True)
    assert raw["iter_num"] == 6 and all(float(s["step"]) == 6.0 for s in raw["optimizer"]["state"].values())
