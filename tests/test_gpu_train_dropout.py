"""Training with dropout on the device (GPT.forward_backward of a config.dropout > 0 model, mgpt_gpt_forward_backward_drop), fp32 path:
gradients against fp64 autograd of the masked restatement (tests/train_dropout_ref.py, masks from sampling.dropout_keep) at trained-like
checkpoints -- peaked attention is where a key / slot mix-up between P and its mask shows --, one site at a time, chunked calls, row0,
determinism, neutrality at p = 0 and in eval mode and a short training run (the training CLI: tests/test_gpu_train_dropout_ddp.py).

The bar is tests/test_gpu_train.py::_check_grads': max|g - g64| <= max(4 x the error of the fp32 autograd of the same masked restatement,
1e-6 max|g64|) and <= 1e-4 max|g64|; the loss to 1e-6 relative."""
import functools

import numpy as np
import pytest
import torch

from mapf_gpt_amd import _lib, weights
from mapf_gpt_amd.model import build_model
from tests import train_dropout_ref as ref
from tests.test_gpu_train import _check_grads, _dev_grads, _kernel_report
from tests.train_ref import LOCALISERS, expert_rows, targets_last, trained_like_state_dict

pytestmark = pytest.mark.gpu

SEED, STEP = 11, 3


@functools.lru_cache(maxsize=None)
def _case(name, rows, case):
    """-> (tokens, targets, trained-like state dict, model args); "last": the expert action at position 255, "all": an id everywhere"""
    args = weights.model_args(LOCALISERS.get(name, name))
    tokens, actions = expert_rows(rows, seed=len(name))
    if case == "last":
        targets = targets_last(actions)
    else:
        targets = np.random.Generator(np.random.PCG64(1)).integers(0, 67, (rows, 256)).astype(np.int64)
    return tokens, targets, trained_like_state_dict(args, 0), args


@functools.lru_cache(maxsize=None)
def _reference(name, rows, case, p, sites=15, row0=0):
    """one fp64 and one fp32 autograd run of the masked restatement per case, shared and left unchanged"""
    tokens, targets, sd, args = _case(name, rows, case)
    l64, g64 = ref.loss_and_grads(sd, args, tokens, targets, p, SEED, STEP, row0, sites, torch.float64)
    _, g32 = ref.loss_and_grads(sd, args, tokens, targets, p, SEED, STEP, row0, sites, torch.float32)
    return l64, g64, g32


def _net(name, rows, case, p, max_rows=4, train_rows=None):
    tokens, targets, sd, args = _case(name, rows, case)
    net = build_model(dict(args, dropout=p), state_dict=sd, max_rows=max_rows)
    net._args = args
    net.set_dropout_rng(SEED, STEP)
    net.train(max_rows=train_rows)
    return net, torch.as_tensor(tokens), torch.as_tensor(targets)


def _check(label, name, got, l64, g64, g32, loss, C):
    assert set(got) == set(g64)
    try:
        _check_grads(label, got, g64, g32)
    except AssertionError as e:
        if name in LOCALISERS:
            raise AssertionError(f"{e}\n{_kernel_report(label, got, g64, g32, C)}") from None
        raise
    print(f"{label}: loss {loss!r} vs fp64 {l64!r}")
    assert abs(loss - l64) <= 1e-6 * abs(l64), (loss, l64)


@pytest.mark.parametrize("case", ["last", "all"])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("name", ["tiny", "1x2x64", "1x4x256", "2M", "6M"])
def test_dropout_gradients_match_fp64_autograd(name, p, case):
    rows = 2 if name == "6M" else 3
    net, tk, tg = _net(name, rows, case, p)
    net.zero_grad()
    loss = float(net.forward_backward(tk, tg, dropout_step=STEP))
    l64, g64, g32 = _reference(name, rows, case, p)
    _check(f"dropout {name} p={p} {case}", name, _dev_grads(net), l64, g64, g32, loss, net._args["n_embd"])


@pytest.mark.parametrize("sites", [1, 2, 4, 8])
@pytest.mark.parametrize("name", list(LOCALISERS))
def test_one_site_at_a_time(name, sites):
    """sites = 1 embedding, 2 attention probabilities, 4 attention's c_proj output, 8 the MLP's: a failure names the broken kernel"""
    net, tk, tg = _net(name, 2, "all", 0.5)
    net.zero_grad()
    loss = float(net.forward_backward(tk, tg, dropout_step=STEP, dropout_sites=sites))
    l64, g64, g32 = _reference(name, 2, "all", 0.5, sites)
    _check(f"dropout {name} sites={sites}", name, _dev_grads(net), l64, g64, g32, loss, net._args["n_embd"])


def test_chunked_call_draws_the_masks_of_the_whole_call():
    """3 rows on a 2-row workspace: a mask keyed by the chunk-local row fails here"""
    net, tk, tg = _net("tiny", 3, "all", 0.5, train_rows=2)
    net.zero_grad()
    loss = float(net.forward_backward(tk, tg, dropout_step=STEP))
    l64, g64, g32 = _reference("tiny", 3, "all", 0.5)
    _check("dropout chunked", "tiny", _dev_grads(net), l64, g64, g32, loss, 64)


def test_row0_splits_a_batch_over_calls():
    """rows 0-1 with row0 = 0 and rows 2-3 with row0 = 2, each at loss_scale 0.5, against the restatement of the 4-row call"""
    net, tk, tg = _net("tiny", 4, "last", 0.5)
    net.zero_grad()
    la = float(net.forward_backward(tk[:2], tg[:2], loss_scale=0.5, dropout_step=STEP, row0=0))
    lb = float(net.forward_backward(tk[2:], tg[2:], loss_scale=0.5, dropout_step=STEP, row0=2))
    l64, g64, g32 = _reference("tiny", 4, "last", 0.5)
    _check_grads("dropout row0", _dev_grads(net), g64, g32)
    assert abs(0.5 * (la + lb) - l64) <= 1e-6 * abs(l64), (la, lb, l64)


def _bits_equal(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


def test_deterministic_and_keyed_by_the_step():
    net, tk, tg = _net("1x4x256", 2, "all", 0.1)
    grads = []
    for step in (STEP, STEP, STEP + 1):
        net.zero_grad()
        net.forward_backward(tk, tg, dropout_step=step)
        grads.append(_dev_grads(net))
    assert _bits_equal(grads[0], grads[1]), "two identical calls differ"
    l64, g64, g32 = _reference("1x4x256", 2, "all", 0.1)
    moved = [k for k, v in g64.items()
             if float((grads[2][k] - grads[0][k]).abs().max()) > max(4 * float((g32[k].double() - v).abs().max()), 1e-6 * float(v.abs().max()))]
    assert moved, "another step changed no tensor by more than its bar"
    # the call counter: set_dropout_rng(seed, step) is used and incremented per call
    net.set_dropout_rng(SEED, STEP)
    for want in (grads[0], grads[2]):
        net.zero_grad()
        net.forward_backward(tk, tg)
        assert _bits_equal(_dev_grads(net), want)
    assert net._drop_step == STEP + 2


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_p0_and_eval_mode_are_the_dropout_free_call(precision):
    net, tk, tg = _net("tiny", 3, "all", 0.1, train_rows=2)
    L, prec = _lib.lib(), _lib.PRECISIONS[precision]
    tok, tgt = tk.to(torch.uint8).cuda().contiguous(), tg.to(torch.int32).cuda().contiguous()
    loss = torch.empty(2, dtype=torch.float32, device="cuda")

    def run(call):
        net.zero_grad()
        call()
        return _dev_grads(net)

    base = run(lambda: _lib.check(L.mgpt_gpt_forward_backward_prec(net._h, _lib.ptr(tok), 3, 256, _lib.ptr(tgt), 1.0, _lib.ptr(loss), prec, _lib.stream_ptr())))
    for p, sites in ((0.0, 15), (0.5, 0)):
        got = run(lambda: _lib.check(L.mgpt_gpt_forward_backward_drop(net._h, _lib.ptr(tok), 3, 256, _lib.ptr(tgt), 1.0, _lib.ptr(loss[1:]), prec, p, 5, 6, 7,
                                                                       sites, _lib.stream_ptr())))
        assert _bits_equal(got, base) and float(loss[0]) == float(loss[1]), (p, sites)
    dropped = run(lambda: net.forward_backward(tk, tg, precision=precision))
    assert not _bits_equal(dropped, base)
    net.eval()
    assert _bits_equal(run(lambda: net.forward_backward(tk, tg, precision=precision)), base)
    net.train()
    assert not _bits_equal(run(lambda: net.forward_backward(tk, tg, precision=precision)), base)
    for p in (1.0, -0.5):
        assert L.mgpt_gpt_forward_backward_drop(net._h, _lib.ptr(tok), 3, 256, _lib.ptr(tgt), 1.0, None, prec, p, 0, 0, 0, 15, _lib.stream_ptr()) == _lib.ERR_ARG


def test_forward_with_targets_stays_dropout_free():
    tokens, targets, sd, args = _case("tiny", 3, "all")
    tk, tg = torch.as_tensor(tokens).cuda(), torch.as_tensor(targets).cuda()
    outs = []
    for p in (0.0, 0.1):
        net = build_model(dict(args, dropout=p), state_dict=sd, max_rows=4)
        net.set_dropout_rng(SEED)
        net.train()
        outs.append(net.forward(tk, tg))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_train_needs_a_pinned_mask_stream():
    """no default seed: train() of a dropout > 0 config raises until set_dropout_rng; a dropout = 0 config needs nothing"""
    tokens, targets, sd, args = _case("tiny", 2, "last")
    net = build_model(dict(args, dropout=0.1), state_dict=sd, max_rows=2)
    with pytest.raises(NotImplementedError, match="set_dropout_rng"):
        net.train()
    net.set_dropout_rng(1)
    assert net.train().training
    float(net.forward_backward(torch.as_tensor(tokens), torch.as_tensor(targets)))
    assert build_model(args, state_dict=sd, max_rows=2).train().training


def test_tiny_learns_expert_rows_with_dropout():
    """The run of test_tiny_learns_expert_rows with dropout = 0.1 beside the dropout-free one: the eval-mode loss on the 388 rows after 20
    steps falls below its starting value and stays within a margin of the dropout-free run's.  A sanity check of sign and scale, not parity.
    First measurement (MI355X): start 4.1994, dropout-free 2.0428, dropout 0.1 2.0441.  The margin 0.05 is 2.5 % of those losses: wide
    against the measured gap of 0.0013, narrow against a wrong scale (s = 1 at p = 0.1 moves the residual branches by 10 %)."""
    tokens, actions = expert_rows(388, seed=7)
    tk, tg = torch.as_tensor(tokens).cuda(), torch.as_tensor(targets_last(actions)).cuda()
    final = {}
    for p in (0.0, 0.1):
        net = build_model(dict(weights.model_args("tiny"), dropout=p), seed=0, max_rows=64)
        net.set_dropout_rng(5)
        net.train()
        opt = net.configure_optimizers(0.1, 1.5e-3, (0.9, 0.95))
        start = float(net.forward(tk, tg)[1])
        for it in range(20):
            sel = np.random.Generator(np.random.PCG64(it)).integers(0, len(tokens), 32)
            net.zero_grad()
            net.forward_backward(torch.as_tensor(tokens[sel]), torch.as_tensor(targets_last(actions[sel])))
            net.clip_grad_norm_(1.0)
            opt.step()
        final[p] = float(net.forward(tk, tg)[1])
        print(f"dropout {p}: eval-mode loss {start:.4f} -> {final[p]:.4f}")
        assert final[p] < 0.8 * start, (p, start, final[p])
    assert abs(final[0.1] - final[0.0]) <= 0.05, final
