"""The last-position micro-step on the device (GPT.forward_backward_rows, mgpt_gpt_forward_backward_rows): rows with one targeted position,
token 255.  It is forward_backward(tokens, targets_last(labels)) with the last layer, ln_f, the head and the cross-entropy on the compact
matrix of the rows' last tokens, so every bar here is the general call's: tests/test_gpu_train.py's _check_grads in fp32 (max(4 x the
fp32-autograd error, 1e-6 max|g|) and <= 1e-4 max|g| of fp64 autograd), tests/test_gpu_train_bf16.py's _check in bf16 (2 x torch autocast's
error + 1e-3 max|g| of fp64 truth)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mapf_gpt_amd import weights
from mapf_gpt_amd.model import GPT, GPTConfig
from tests.test_gpu_train import _check_grads, _dev_grads, _rows, _trained_net
from tests.test_gpu_train_bf16 import _check, _ref
from tests.train_ref import LOCALISERS, loss_and_grads, targets_last, targets_mixed, trained_like_state_dict

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _n_rows(name):
    return 2 if name == "85M" else 3


@functools.lru_cache(maxsize=None)
def _case(name, rows, trained):
    """(tokens, labels, state dict, model args) of a case: expert rows, synthetic N(0, 0.02) weights or the trained-like checkpoint"""
    args = weights.model_args(LOCALISERS.get(name, name))
    tokens, labels = _rows(rows, seed=len(name))
    sd = trained_like_state_dict(args) if trained else weights.synthetic_state_dict(args, seed=0)
    return tokens, labels, sd, args


@functools.lru_cache(maxsize=None)
def _ref_f32(name, rows, trained):
    """one fp64 and one fp32 autograd run per case on last-only targets, shared and left unchanged"""
    tokens, labels, sd, args = _case(name, rows, trained)
    l64, g64 = loss_and_grads(sd, args, tokens, targets_last(labels), torch.float64)
    _, g32 = loss_and_grads(sd, args, tokens, targets_last(labels), torch.float32)
    return l64, g64, g32


@functools.lru_cache(maxsize=None)
def _ref_bf16(name, rows, trained):
    tokens, labels, sd, args = _case(name, rows, trained)
    micro = [(tokens, targets_last(labels))]
    l64, g64 = _ref(sd, args, micro)
    lac, gac = _ref(sd, args, micro, autocast=True)
    return l64[0], g64, lac[0], gac


def _model(name, rows, trained, train_rows=None):
    tokens, labels, sd, args = _case(name, rows, trained)
    return _trained_net(args, sd, max_rows=max(4, train_rows or rows), train_rows=train_rows or max(4, rows))


def _run(net, tokens, labels, precision="f32", **kw):
    net.zero_grad()
    loss = float(net.forward_backward_rows(torch.as_tensor(tokens), torch.as_tensor(labels), precision=precision, **kw))
    return loss, _dev_grads(net)


def _check_f32(tag, name, rows, trained, train_rows=None):
    tokens, labels, _, _ = _case(name, rows, trained)
    l64, g64, g32 = _ref_f32(name, rows, trained)
    loss, got = _run(_model(name, rows, trained, train_rows), tokens, labels)
    assert set(got) == set(g64)
    _check_grads(tag, got, g64, g32)
    print(f"{tag}: loss {loss!r}, fp64 {l64!r}")
    assert abs(loss - l64) <= 1e-5 * abs(l64), (loss, l64)
    return loss


def _check_bf16(tag, name, rows, trained, train_rows=None):
    tokens, labels, _, _ = _case(name, rows, trained)
    l64, g64, lac, gac = _ref_bf16(name, rows, trained)
    loss, got = _run(_model(name, rows, trained, train_rows), tokens, labels, precision="bf16")
    _check(tag, got, g64, gac, loss, l64, lac)


@pytest.mark.parametrize("name", ["tiny", "2M", "6M", "85M"])
def test_rows_gradients_match_fp64_autograd(name):
    _check_f32(f"rows {name}", name, _n_rows(name), False)


@pytest.mark.parametrize("name", ["tiny", "6M", *LOCALISERS])
def test_rows_trained_like_gradients_match_fp64_autograd(name):
    """peaked attention: at N(0, 0.02) it is nearly uniform and a key mix-up in the token-255 attention kernels would hide"""
    _check_f32(f"rows trained-like {name}", name, 3, True)


@pytest.mark.parametrize("name,trained", [("tiny", False), ("2M", False), ("6M", False), ("6M", True), ("1x4x256", True)])
def test_rows_bf16_within_the_autocast_bar(name, trained):
    _check_bf16(f"rows bf16 {name}{' trained-like' if trained else ''}", name, 3, trained)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("rows", [1, 17, 33, 65])
def test_rows_ragged_compact_counts(rows, precision):
    """compact token counts off the weight-gradient slabs' 16- and 32-token alignment, one chunk each"""
    (_check_f32 if precision == "f32" else _check_bf16)(f"rows {precision} {rows} rows", "tiny", rows, True, train_rows=rows)


def test_rows_chunked_call_matches_one_chunk():
    """5 rows in chunks of 2, 2, 1: the normaliser is the whole call's row count"""
    _check_f32("rows chunked", "tiny", 5, True, train_rows=2)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_rows_deterministic(precision):
    tokens, labels, _, _ = _case("6M", 4, False)
    net = _model("6M", 4, False)
    la, a = _run(net, tokens, labels, precision)
    lb, b = _run(net, tokens, labels, precision)
    assert la == lb
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k}: two identical {precision} calls differ"


def test_rows_mix_with_the_general_call():
    """one general micro-step (mixed targets) and one rows micro-step, loss_scale 0.5 each, into the same gradient buffer"""
    tokens, labels, sd, args = _case("tiny", 4, True)
    t1, a1 = tokens[:2], targets_mixed(2)
    t2, a2 = tokens[2:], targets_last(labels[2:])
    net = _model("tiny", 4, True)
    net.zero_grad()
    net.forward_backward(torch.as_tensor(t1), torch.as_tensor(a1), loss_scale=0.5)
    net.forward_backward_rows(torch.as_tensor(t2), torch.as_tensor(labels[2:]), loss_scale=0.5)
    got = _dev_grads(net)
    _, g64 = loss_and_grads(sd, args, None, None, torch.float64, 0.5, micro=[(t1, a1), (t2, a2)])
    _, g32 = loss_and_grads(sd, args, None, None, torch.float32, 0.5, micro=[(t1, a1), (t2, a2)])
    _check_grads("rows mixed with general", got, g64, g32)


@pytest.mark.parametrize("name", ["tiny", "2M"])
def test_rows_loss_equals_the_general_call(name):
    tokens, labels, _, _ = _case(name, 3, False)
    net = _model(name, 3, False)
    loss, _ = _run(net, tokens, labels)
    net.zero_grad()
    general = float(net.forward_backward(torch.as_tensor(tokens), torch.as_tensor(targets_last(labels))))
    assert abs(loss - general) <= 1e-6 * abs(general), (loss, general)


def test_rows_refusals_and_guards():
    tokens, labels, sd, args = _case("tiny", 3, False)
    tk = torch.as_tensor(tokens)
    cold = GPT(GPTConfig(**args), max_rows=4)
    cold.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="train"):
        cold.forward_backward_rows(tk, torch.as_tensor(labels))
    net = _model("tiny", 3, False)
    net.zero_grad()
    for bad in (67, -1):
        lb = np.array(labels)
        lb[1] = bad
        with pytest.raises(ValueError, match="labels must lie"):
            net.forward_backward_rows(tk, torch.as_tensor(lb))
    assert all(float(v.abs().max()) == 0.0 for v in _dev_grads(net).values())       # refused before any launch
    with pytest.raises(ValueError):
        net.forward_backward_rows(tk, torch.as_tensor(labels[:2]))
    with pytest.raises(ValueError):
        net.forward_backward_rows(tk[:, :255], torch.as_tensor(labels))
    with pytest.raises(ValueError):
        net.forward_backward_rows(tk, torch.as_tensor(targets_last(labels)))
    with pytest.raises(RuntimeError, match="precision"):
        net.forward_backward_rows(tk, torch.as_tensor(labels), precision="f16x3")
    drop = GPT(GPTConfig(**dict(args, dropout=0.1)), max_rows=4)
    drop.load_state_dict(sd)
    drop.set_dropout_rng(1)
    drop.train()
    with pytest.raises(NotImplementedError, match="forward_backward"):
        drop.forward_backward_rows(tk, torch.as_tensor(labels))
    drop.eval()
    assert np.isfinite(float(drop.forward_backward_rows(tk, torch.as_tensor(labels))))


def test_rows_out_of_range_device_label_is_nan_not_a_fault():
    """check=False: the cross-entropy kernel compares the label with [0, 67) before it indexes with it; the row's loss term is NaN and the
    other rows are computed as ever (the logits of the same rows through the scoring path stay finite and equal)."""
    tokens, labels, _, _ = _case("tiny", 3, False)
    net = _model("tiny", 3, False)
    lb = torch.as_tensor(np.array(labels)).cuda()
    lb[1] = 67
    net.zero_grad()
    loss = net.forward_backward_rows(torch.as_tensor(tokens).cuda(), lb, check=False)
    assert bool(torch.isnan(loss))
    assert bool(torch.isnan(net.clip_grad_norm_(1.0)))
    good, _ = _run(net, tokens, labels)
    assert np.isfinite(good)
    l64, _, _ = _ref_f32("tiny", 3, False)
    assert abs(good - l64) <= 1e-5 * abs(l64)


def _write_shards(d, n_files=2, rows=24):
    from mapf_gpt_amd.dataset_build import write_arrow
    tokens, labels = _rows(n_files * rows, seed=11)
    for i in range(n_files):
        write_arrow(os.path.join(d, f"part_{i}.arrow"), tokens[i * rows:(i + 1) * rows].astype(np.int8), labels[i * rows:(i + 1) * rows])


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_rows_call_training_cli(tmp_path, dtype):
    """python -m mapf_gpt_amd.training --rows-call against the same command without it: the same data order, so the final losses differ by
    summation order only"""
    pytest.importorskip("pyarrow")
    data = tmp_path / "data"
    data.mkdir()
    _write_shards(str(data))
    final = {}
    for flag in ((), ("--rows-call",)):
        out = tmp_path / ("rows" if flag else "general")
        cmd = [sys.executable, "-m", "mapf_gpt_amd.training", "--init", "tiny", "--data", str(data), "--val", str(data), "--out-dir", str(out),
               "--max-iters", "4", "--eval-interval", "2", "--eval-iters", "1", "--batch-size", "4", "--gradient-accumulation-steps", "2",
               "--dtype", dtype, *flag]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        final[bool(flag)] = json.loads(r.stdout.strip().splitlines()[-1])["loss"]
        args, sd = weights.load_checkpoint(str(out / "ckpt.pt"))
        assert args["n_layer"] == 2 and "transformer.wte.weight" in sd
    print(f"{dtype}: final loss general {final[False]!r}, rows call {final[True]!r}")
    assert abs(final[True] - final[False]) <= 1e-4 * abs(final[False]), final
