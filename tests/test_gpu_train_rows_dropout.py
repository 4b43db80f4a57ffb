"""The last-position micro-step with dropout on the device (GPT.forward_backward_rows_drop, mgpt_gpt_forward_backward_rows_drop): it is
forward_backward(tokens, targets_last(labels)) of a config.dropout > 0 model with the same seed, step, row0 and sites -- the compact last
layer draws the general call's masks at token / query 255 -- so every bar here is the general call's with dropout:
fp32  tests/test_gpu_train_dropout.py's _check (= _check_grads against fp64 and fp32 autograd of the masked restatement; loss to 1e-6);
bf16  tests/test_gpu_train_bf16.py's _check (2 x torch autocast's error on the masked restatement with the same masks + 1e-3 max|g64|).
The references are those of tests/test_gpu_train_dropout.py and tests/test_gpu_train_dropout_bf16.py on their "last" case (cached there
and shared); the trained-like checkpoints have peaked attention, where a key / slot mix-up between P and its mask cannot hide."""
import json
import subprocess
import sys

import numpy as np
import pytest
import torch

from mapf_gpt_amd import _lib, weights
from tests import train_dropout_ref as ref
from tests.helpers import ROOT
from tests.test_gpu_train import _check_grads, _dev_grads
from tests.test_gpu_train_bf16 import _check as _check_bf16
from tests.test_gpu_train_dropout import SEED, STEP, _bits_equal, _case, _check, _net, _reference
from tests.test_gpu_train_dropout_bf16 import _reference as _reference_bf16
from tests.test_gpu_train_rows import _write_shards
from tests.train_ref import LOCALISERS, targets_mixed

pytestmark = pytest.mark.gpu


def _rows_net(name, rows, p, train_rows=None):
    """-> (net in training mode, tokens, labels, targets_last(labels)); the workspace holds train_rows rows (default: every row, one chunk)"""
    net, tk, tg = _net(name, rows, "last", p, max_rows=max(4, rows), train_rows=train_rows or max(4, rows))
    return net, tk, tg[:, -1].clone(), tg


def _run(net, tk, lb, precision="f32", **kw):
    net.zero_grad()
    kw.setdefault("dropout_step", STEP)
    loss = float(net.forward_backward_rows_drop(tk, lb, precision=precision, **kw))
    return loss, _dev_grads(net)


def _check_case(tag, name, rows, p, precision, sites=15, train_rows=None):
    net, tk, lb, _ = _rows_net(name, rows, p, train_rows)
    loss, got = _run(net, tk, lb, precision, dropout_sites=sites)
    key = (name, rows, "last", p) if sites == 15 else (name, rows, "last", p, sites)      # (the cache key of the general call's tests)
    if precision == "f32":
        l64, g64, g32 = _reference(*key)
        _check(tag, name, got, l64, g64, g32, loss, net._args["n_embd"])
    else:
        l64, g64, lac, gac = _reference_bf16(*key)
        _check_bf16(tag, got, g64, gac, loss, l64, lac)
    return net, tk, lb, loss, got


CASES = [(n, p) for n in ("tiny", *LOCALISERS) for p in (0.1, 0.5)] + [("6M", 0.1)]


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("name,p", CASES)
def test_rows_drop_gradients_within_the_general_calls_bar(name, p, precision):
    _check_case(f"rows drop {precision} {name} p={p}", name, 2 if name == "6M" else 3, p, precision)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("sites", [1, 2, 4, 8])
@pytest.mark.parametrize("name", list(LOCALISERS))
def test_rows_drop_one_site_at_a_time(name, sites, precision):
    """a one-layer model is all compact code fed by a masked embedding: sites = 1 embedding, 2 attention probabilities (attn_last_*_kernel),
    4 attention's c_proj output, 8 the MLP's (the compact residual joins) -- a failure names the broken kernel"""
    _check_case(f"rows drop {precision} {name} sites={sites}", name, 2, 0.5, precision, sites)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["tiny", "1x4x256"])
def test_rows_drop_against_the_general_call(name, precision):
    """the same seed, step, row0 and sites through both calls: both within their bars of the same fp64 truth, the fp32 losses equal to 1e-6"""
    net, tk, lb, loss, _ = _check_case(f"rows drop vs general {precision} {name}", name, 3, 0.1, precision)
    _, _, _, tg = _rows_net(name, 3, 0.1)
    net.zero_grad()
    general = float(net.forward_backward(tk, tg, precision=precision, dropout_step=STEP))
    got = _dev_grads(net)
    if precision == "f32":
        l64, g64, g32 = _reference(name, 3, "last", 0.1)
        _check(f"general {name}", name, got, l64, g64, g32, general, net._args["n_embd"])
        assert abs(loss - general) <= 1e-6 * abs(general), (loss, general)
    else:
        l64, g64, lac, gac = _reference_bf16(name, 3, "last", 0.1)
        _check_bf16(f"general bf16 {name}", got, g64, gac, general, l64, lac)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("rows", [1, 17, 33])
def test_rows_drop_ragged_compact_counts(rows, precision):
    """compact token counts off the 16- and 32-token alignments, one chunk each: in bf16 the padding rows of the compact matrix stay zero
    under the masks (the residual-join epilogue and the masked gradient run over them)"""
    _check_case(f"rows drop {precision} {rows} rows", "tiny", rows, 0.5, precision, train_rows=rows)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_rows_drop_chunked_call_draws_the_masks_of_the_whole_call(precision):
    """5 rows on a 2-row workspace: a mask keyed by the chunk-local row fails here"""
    _check_case(f"rows drop {precision} chunked", "tiny", 5, 0.5, precision, train_rows=2)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_rows_drop_row0_splits_a_batch_over_calls(precision):
    """rows 0-1 with row0 = 0 and rows 2-3 with row0 = 2, each at loss_scale 0.5, against the restatement of the 4-row call"""
    net, tk, lb, _ = _rows_net("tiny", 4, 0.5)
    net.zero_grad()
    la = float(net.forward_backward_rows_drop(tk[:2], lb[:2], loss_scale=0.5, precision=precision, dropout_step=STEP, row0=0))
    lb_ = float(net.forward_backward_rows_drop(tk[2:], lb[2:], loss_scale=0.5, precision=precision, dropout_step=STEP, row0=2))
    got = _dev_grads(net)
    if precision == "f32":
        l64, g64, g32 = _reference("tiny", 4, "last", 0.5)
        _check_grads("rows drop row0", got, g64, g32)
        assert abs(0.5 * (la + lb_) - l64) <= 1e-6 * abs(l64), (la, lb_, l64)
    else:
        l64, g64, lac, gac = _reference_bf16("tiny", 4, "last", 0.5)
        _check_bf16("rows drop bf16 row0", got, g64, gac, 0.5 * (la + lb_), l64, lac)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_rows_drop_deterministic_keyed_by_the_step_and_counted(precision):
    net, tk, lb, _ = _rows_net("1x4x256", 3, 0.1)
    grads = [_run(net, tk, lb, precision, dropout_step=step)[1] for step in (STEP, STEP, STEP + 1)]
    assert _bits_equal(grads[0], grads[1]), "two identical calls differ"
    # another step moves at least one tensor by more than its bar
    if precision == "f32":
        _, g64, g32 = _reference("1x4x256", 3, "last", 0.1)
        bar = {k: max(4 * float((g32[k].double() - v).abs().max()), 1e-6 * float(v.abs().max())) for k, v in g64.items()}
    else:
        _, g64, _, gac = _reference_bf16("1x4x256", 3, "last", 0.1)
        bar = {k: 2 * float((gac[k] - v).abs().max()) + 1e-3 * float(v.abs().max()) for k, v in g64.items()}
    moved = [k for k in g64 if float((grads[2][k] - grads[0][k]).abs().max()) > bar[k]]
    assert moved, "another step changed no tensor by more than its bar"
    # the call counter: set_dropout_rng(seed, step) is used and incremented per call; an explicit dropout_step leaves it alone
    net.set_dropout_rng(SEED, STEP)
    for want in (grads[0], grads[2]):
        net.zero_grad()
        net.forward_backward_rows_drop(tk, lb, precision=precision)
        assert _bits_equal(_dev_grads(net), want)
    assert net._drop_step == STEP + 2
    _run(net, tk, lb, precision, dropout_step=STEP)
    assert net._drop_step == STEP + 2


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_rows_drop_p0_sites0_and_eval_mode_are_the_rows_call(precision):
    """bit equality with forward_backward_rows: p = 0 and sites = 0 through the new entry point, and the new method after eval()"""
    net, tk, lb, _ = _rows_net("tiny", 3, 0.1, train_rows=2)
    L, prec = _lib.lib(), _lib.PRECISIONS[precision]
    tok, lab = tk.to(torch.uint8).cuda().contiguous(), lb.to(torch.int32).cuda().contiguous()
    loss = torch.empty(2, dtype=torch.float32, device="cuda")

    def run(call):
        net.zero_grad()
        call()
        return _dev_grads(net)

    base = run(lambda: _lib.check(L.mgpt_gpt_forward_backward_rows(net._h, _lib.ptr(tok), 3, _lib.ptr(lab), 1.0, _lib.ptr(loss), prec, _lib.stream_ptr())))
    for p, sites in ((0.0, 15), (0.5, 0)):
        got = run(lambda: _lib.check(L.mgpt_gpt_forward_backward_rows_drop(net._h, _lib.ptr(tok), 3, _lib.ptr(lab), 1.0, _lib.ptr(loss[1:]), prec, p, 5, 6, 7,
                                                                            sites, _lib.stream_ptr())))
        assert _bits_equal(got, base) and float(loss[0]) == float(loss[1]), (p, sites)
    assert not _bits_equal(run(lambda: net.forward_backward_rows_drop(tk, lb, precision=precision)), base)
    net.eval()
    assert _bits_equal(run(lambda: net.forward_backward_rows_drop(tk, lb, precision=precision)), base)
    assert _bits_equal(run(lambda: net.forward_backward_rows(tk, lb, precision=precision)), base)
    net.train()
    assert not _bits_equal(run(lambda: net.forward_backward_rows_drop(tk, lb, precision=precision)), base)
    with pytest.raises(NotImplementedError):                       # the dropout-free method refuses as it did
        net.forward_backward_rows(tk, lb, precision=precision)
    for p in (1.0, -0.5):
        assert L.mgpt_gpt_forward_backward_rows_drop(net._h, _lib.ptr(tok), 3, _lib.ptr(lab), 1.0, None, prec, p, 0, 0, 0, 15, _lib.stream_ptr()) == _lib.ERR_ARG
    assert L.mgpt_gpt_forward_backward_rows_drop(net._h, _lib.ptr(tok), 3, _lib.ptr(lab), 1.0, None, prec, 0.1, 0, 0, 0, 16, _lib.stream_ptr()) == _lib.ERR_ARG


def test_rows_drop_out_of_range_device_label_is_nan_not_a_fault():
    """check=False: the cross-entropy kernel compares the label with [0, 67) before it indexes with it; the loss is NaN and the next call is
    what it would have been"""
    net, tk, lb, _ = _rows_net("tiny", 3, 0.1)
    bad = lb.clone().cuda()
    bad[1] = 67
    net.zero_grad()
    loss = net.forward_backward_rows_drop(tk.cuda(), bad, check=False, dropout_step=STEP)
    assert bool(torch.isnan(loss))
    assert bool(torch.isnan(net.clip_grad_norm_(1.0)))
    with pytest.raises(ValueError, match="labels must lie"):
        net.forward_backward_rows_drop(tk, bad.cpu(), dropout_step=STEP)
    good, got = _run(net, tk, lb)
    l64, g64, g32 = _reference("tiny", 3, "last", 0.1)
    _check("rows drop after a NaN call", "tiny", got, l64, g64, g32, good, 64)


def test_rows_drop_mixes_with_the_general_dropout_call():
    """one general dropout micro-step (mixed targets, rows 0-1) and one rows-drop micro-step (rows 2-3, row0 = 2), loss_scale 0.5 each, into
    one gradient buffer"""
    tokens, targets, sd, args = _case("tiny", 4, "last")
    net, tk, lb, _ = _rows_net("tiny", 4, 0.5)
    a1 = targets_mixed(2)
    net.zero_grad()
    net.forward_backward(tk[:2], torch.as_tensor(a1), loss_scale=0.5, dropout_step=STEP, row0=0)
    net.forward_backward_rows_drop(tk[2:], lb[2:], loss_scale=0.5, dropout_step=STEP, row0=2)
    got = _dev_grads(net)
    micro = [(tokens[:2], a1, 0), (tokens[2:], targets[2:], 2)]
    _, g64 = ref.loss_and_grads(sd, args, None, None, 0.5, SEED, STEP, dtype=torch.float64, loss_scale=0.5, micro=micro)
    _, g32 = ref.loss_and_grads(sd, args, None, None, 0.5, SEED, STEP, dtype=torch.float32, loss_scale=0.5, micro=micro)
    _check_grads("rows drop mixed with general", got, g64, g32)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_rows_call_drop_training_cli(tmp_path, dtype):
    """python -m mapf_gpt_amd.training --dropout 0.1 with and without --rows-call-drop: the same data order and the same masks, so the final
    losses differ by summation order only (the relative bar of test_rows_call_training_cli)"""
    pytest.importorskip("pyarrow")
    data = tmp_path / "data"
    data.mkdir()
    _write_shards(str(data))
    final = {}
    for flag in ((), ("--rows-call-drop",)):
        out = tmp_path / ("rows" if flag else "general")
        cmd = [sys.executable, "-m", "mapf_gpt_amd.training", "--init", "tiny", "--data", str(data), "--val", str(data), "--out-dir", str(out),
               "--max-iters", "4", "--eval-interval", "2", "--eval-iters", "1", "--batch-size", "4", "--gradient-accumulation-steps", "2",
               "--dtype", dtype, "--dropout", "0.1", *flag]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        final[bool(flag)] = json.loads(r.stdout.strip().splitlines()[-1])["loss"]
        args, _ = weights.load_checkpoint(str(out / "ckpt.pt"))
        assert args["n_layer"] == 2 and args["dropout"] == 0.1
    print(f"{dtype}: final loss general {final[False]!r}, rows-call-drop {final[True]!r}")
    assert np.isfinite(final[True])
    assert abs(final[True] - final[False]) <= 1e-4 * abs(final[False]), final
