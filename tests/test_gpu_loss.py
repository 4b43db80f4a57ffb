"""GPT.forward(idx, targets), GPT.score_tokens and mapf_gpt_amd/scoring.py on the device (mgpt_gpt_forward_seq / mgpt_gpt_score_last):
logits of every position and the cross-entropy against the pinned oracle's restatement of model.py:178-184, in every precision and call
regime; scoring hits bit-identical to act; the default forward undisturbed by a sequence forward before it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mapf_gpt_amd import weights
from mapf_gpt_amd.model import build_model
from tests.helpers import GOLDEN, ROOT
from tests.test_loss_cpu import seq_oracle

pytestmark = pytest.mark.gpu

TOL = 1e-5
PROBE_TOL, PROBE_REL = 1e-5, 7.62939453125e-6     # include/mapf_gpt_amd.h MGPT_ENVELOPE_PROBE_TOL / _REL


def _targets(rows, T, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    t = rng.integers(0, 67, (rows, T)).astype(np.int64)
    t[rng.random((rows, T)) < 0.3] = -1
    if rows > 1:
        t[1] = -1
        t[1, T - 1] = rng.integers(0, 5)
    return t


def _seq(net, tokens, targets):
    logits, loss = net(torch.as_tensor(tokens).cuda(), torch.as_tensor(targets).cuda())
    return logits.cpu().numpy(), float(loss)


def _check_rows(net, name, tokens, targets, rows_cmp, bar, loss_rel, dtype=torch.float64):
    """forward(idx, targets) on all `tokens`; compare the rows `rows_cmp` (every position) and their cross-entropy with the oracle"""
    logits, loss_all = _seq(net, tokens, targets)
    sd = net._sd
    # the kernel's cross-entropy in this call regime against F.cross_entropy of its own logits
    ce = torch.nn.functional.cross_entropy(torch.from_numpy(logits).double().reshape(-1, 67), torch.as_tensor(targets).long().reshape(-1), ignore_index=-1)
    assert abs(loss_all - float(ce)) <= 1e-5 * abs(float(ce)), (name, loss_all, float(ce))
    ref, _ = seq_oracle(sd, net._args, tokens[rows_cmp], None, dtype=dtype)
    ref = ref.numpy()
    err = float(np.abs(logits[rows_cmp] - ref).max())
    b = bar(ref) if callable(bar) else bar
    assert err <= b, f"{name}: logits of every position differ by {err:.3e} (bar {b:.3e})"
    # loss of the compared rows alone: the library's row sums against F.cross_entropy
    sub = torch.as_tensor(targets[rows_cmp])
    _, loss = _seq(net, tokens[rows_cmp], sub)
    _, ref_loss = seq_oracle(sd, net._args, tokens[rows_cmp], sub, dtype=dtype)
    assert abs(loss - float(ref_loss)) <= loss_rel * abs(float(ref_loss)), (name, loss, float(ref_loss))
    return err


def _net(name, precision="f32", max_rows=16, seed=0, scale=1.0, args=None):
    a = weights.model_args(args if args is not None else name)
    sd = weights.synthetic_state_dict(a, seed=seed, scale=scale)
    net = build_model(a, max_rows=max_rows, precision=precision, state_dict=sd)
    net._sd, net._args = sd, a
    return net


def test_library_matches_reference_golden():
    for name in ("tiny", "6M"):
        g = np.load(os.path.join(GOLDEN, f"loss_{name}.npz"))
        net = _net(name, seed=int(g["seed"]), scale=float(g["scale"]), max_rows=4)
        logits, loss = _seq(net, g["tokens"], g["targets"])
        err = float(np.abs(logits[:, g["positions"], :] - g["logits"]).max())
        assert err <= TOL, f"{name}: {err:.3e}"
        assert abs(loss - float(g["loss"])) <= TOL * abs(float(g["loss"])), (loss, float(g["loss"]))


@pytest.mark.parametrize("name", ["tiny", "2M", "6M", "85M", "6M_bias"])
def test_f32_every_position_vs_oracle(name):
    shape = name.split("_")[0]
    args = dict(weights.MODEL_SHAPES[shape], bias=name.endswith("bias"))
    net = _net(shape, max_rows=4, args=args)
    rng = np.random.Generator(np.random.PCG64(11))
    rows = 2 if shape == "85M" else 3
    tok = rng.integers(0, 67, (rows, 256)).astype(np.uint8)
    _check_rows(net, name, tok, _targets(rows, 256, 1), np.arange(rows), TOL, TOL, dtype=torch.float32)
    for T in (1, 37, 161):                        # rows shorter than 256 tokens (exact-fp32 kernels, plain residual layout)
        tok = rng.integers(0, 67, (2, T)).astype(np.uint8)
        _check_rows(net, f"{name} T={T}", tok, _targets(2, T, T), np.arange(2), TOL, TOL, dtype=torch.float32)


def _e_last_bf16(shape, g, rows):
    """the existing bf16 forward's own max error against fp64 at position 255 on the same rows"""
    net = build_model(shape, seed=int(g["seed"]), scale=float(g["scale"]), max_rows=16, precision="bf16")
    got = net.logits_tokens(torch.from_numpy(g["tokens"][rows]).cuda()).cpu().numpy()
    return float(np.abs(got - g["logits_f64"][rows]).max())


# (shape, max_rows, [call sizes]): <= 128 rows (small kernels), 512 rows, and max_rows + 37 (ragged chunking); 85M with fewer rows
REGIMES = {"2M": (256, [8, 512, 293]), "6M": (256, [8, 512, 293]), "85M": (96, [4, 160, 133])}


@pytest.mark.parametrize("precision", ["f16x3", "bf16"])
@pytest.mark.parametrize("shape", ["2M", "6M", "85M"])
def test_16bit_every_position_every_regime(shape, precision):
    g = np.load(os.path.join(GOLDEN, f"gptbig_{shape}_s1.npz"))
    max_rows, calls = REGIMES[shape]
    net = _net(shape, precision=precision, max_rows=max_rows, seed=int(g["seed"]), scale=float(g["scale"]))
    n_cmp = 2 if shape == "85M" else 3
    if precision == "bf16":
        e_last = _e_last_bf16(shape, g, np.arange(n_cmp))
        bar = 1.5 * e_last + 2e-3
    else:
        bar = lambda ref: max(PROBE_TOL, PROBE_REL * float(np.abs(ref).max()))     # gpt.hip envelope_decide
    base = g["tokens"]
    for n in calls:
        tok = np.concatenate([base] * ((n + 255) // 256))[:n]
        tok = np.roll(tok, -(n % 7), axis=0)                  # other rows first in every call
        tg = _targets(n, 256, n)
        cmp = np.array([0, 1, n - 1])[:n_cmp] if n > 2 else np.arange(n)
        _check_rows(net, f"{shape} {precision} {n} rows", tok, tg, cmp, bar, 1e-3 if precision == "bf16" else 1e-4)
    assert net.envelope()["effective_precision"] == "f16x3" or precision == "bf16"


@pytest.mark.parametrize("precision", ["f32", "f16x3", "bf16"])
@pytest.mark.parametrize("shape", ["2M", "6M"])
def test_score_hits_equal_act_and_nll_matches_oracle(shape, precision):
    from mapf_gpt_amd import scoring
    net = _net(shape, precision=precision, max_rows=100, seed=2)
    for ds in ("ds_random", "ds_maze"):
        d = np.load(os.path.join(GOLDEN, f"{ds}.npz"))
        x, y = d["inputs"], d["gt_actions"].astype(np.int64)
        tok = torch.from_numpy(x.astype(np.uint8)).cuda()
        for n in (64, x.shape[0]):                       # one small call, one large call chunked at max_rows = 100
            nll, hit = net.score_tokens(tok[:n], torch.from_numpy(y[:n]))
            act = net.act_tokens(tok[:n], do_sample=False).cpu().numpy()
            assert np.array_equal(hit.cpu().numpy(), act == y[:n]), (ds, n)
            lg = net.logits_tokens(tok[:n]).cpu().numpy()
            ce = -torch.log_softmax(torch.from_numpy(lg).double(), -1)[torch.arange(n), torch.from_numpy(y[:n])].numpy()
            assert np.abs(nll.cpu().numpy() - ce).max() <= 2e-6 * max(1.0, float(np.abs(ce).max())), (ds, n)
            ref, _ = seq_oracle(net._sd, net._args, x[:2].astype(np.int64), None, dtype=torch.float64)
            ref_ce = -torch.log_softmax(ref[:, -1, :], -1)[torch.arange(2), torch.from_numpy(y[:2])].numpy()
            bar = 2e-2 if precision == "bf16" else max(PROBE_TOL, PROBE_REL * float(ref.abs().max())) * 2
            assert np.abs(nll.cpu().numpy()[:2] - ref_ce).max() <= bar, (ds, n, precision)
        res = scoring.evaluate(net, x, y)                # (one call of every row: the same kernels as the score_tokens call below)
        nll, hit = net.score_tokens(tok, torch.from_numpy(y))
        assert res["rows"] == x.shape[0]
        assert abs(res["loss"] - float(nll.double().mean())) <= 1e-6 * max(1.0, abs(res["loss"]))
        assert res["accuracy"] == float(hit.double().mean())
        assert res["effective_precision"] == precision


@pytest.mark.parametrize("shape,precision", [("2M", "f16x3"), ("2M", "bf16"), ("6M", "f16x3"), ("6M", "bf16"), ("85M", "bf16"), ("tiny", "f16x3")])
def test_sequence_forward_leaves_the_default_path_undisturbed(shape, precision):
    rng = np.random.Generator(np.random.PCG64(4))
    max_rows = 64 if shape == "85M" else 160
    big = 150 if shape == "85M" else 300
    tok = torch.from_numpy(rng.integers(0, 67, (big, 256)).astype(np.uint8)).cuda()
    gt = torch.from_numpy(rng.integers(0, 5, big))
    fresh = _net(shape, precision=precision, max_rows=max_rows, seed=6)
    used = _net(shape, precision=precision, max_rows=max_rows, seed=6)
    for n in (8, big):
        used(tok[:n], torch.from_numpy(_targets(n, 256, 3)))
        used.score_tokens(tok[:n], gt[:n])
    for n in (8, big):
        a = fresh.logits_tokens(tok[:n]).cpu().numpy()
        b = used.logits_tokens(tok[:n]).cpu().numpy()
        assert np.array_equal(a, b), (shape, precision, n)
        assert np.array_equal(fresh.act_tokens(tok[:n], do_sample=False).cpu().numpy(), used.act_tokens(tok[:n], do_sample=False).cpu().numpy())


def test_python_surface():
    net = _net("tiny", max_rows=8)
    idx = torch.randint(0, 67, (3, 256))
    logits, loss = net(idx, torch.full((3 * 256,), -1, dtype=torch.int64))     # any shape with numel B * T (targets.view(-1))
    assert logits.shape == (3, 256, 67) and logits.dtype == torch.float32 and loss.dim() == 0 and loss.dtype == torch.float32
    assert torch.isnan(loss)                                                     # every target ignored: 0 / 0, as F.cross_entropy
    t = torch.full((3, 256), -1, dtype=torch.int8)
    t[:, -1] = 2
    _, loss = net(idx, t)
    assert torch.isfinite(loss)
    logits, loss = net(idx[:, :40], torch.zeros(3, 40, dtype=torch.int32))       # T < 256
    assert logits.shape == (3, 40, 67) and torch.isfinite(loss)
    for bad in (67, -2):
        t = torch.zeros(3, 256, dtype=torch.int64)
        t[1, 7] = bad
        with pytest.raises(ValueError):
            net(idx, t)
    with pytest.raises(ValueError):
        net(idx, torch.zeros(3, 255, dtype=torch.int64))
    lg1, none = net(idx)                                                         # without targets: unchanged
    assert lg1.shape == (3, 1, 67) and none is None


def test_scoring_cli(tmp_path):
    pa = pytest.importorskip("pyarrow")
    a = weights.model_args("tiny")
    sd = weights.synthetic_state_dict(a, seed=1)
    ckpt = tmp_path / "ckpt.pt"
    torch.save({"model": {"_orig_mod." + k: torch.from_numpy(v) for k, v in sd.items()}, "model_args": a}, str(ckpt))
    d = np.load(os.path.join(GOLDEN, "ds_random.npz"))
    table = pa.table({"input_tensors": pa.array(list(d["inputs"])), "gt_actions": pa.array(d["gt_actions"])})
    with pa.OSFile(str(tmp_path / "val.arrow"), "wb") as sink:
        with pa.ipc.new_file(sink, table.schema) as w:
            w.write_table(table)
    r = subprocess.run([sys.executable, "-m", "mapf_gpt_amd.scoring", "--weights", str(ckpt), "--data", str(tmp_path / "val.arrow"),
                        "--precision", "f32", "--batch-size", "64"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["rows"] == d["inputs"].shape[0] and out["effective_precision"] == "f32" and np.isfinite(out["loss"]) and 0 <= out["accuracy"] <= 1
    assert out["rows_per_s"] > 0
