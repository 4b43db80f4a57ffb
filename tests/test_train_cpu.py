"""CPU checks of the training CLI (mapf_gpt_amd/training.py): its learning-rate schedule against a restatement of train.py:263-276 and its
batches against a restatement of fast_data_loader.py:39-67 with train.py:162-165 (targets -1 except the last position, a per-file shuffle);
and of the trained-like checkpoint recipe of the device gradient tests (tests/train_ref.py) against the fp64 oracle."""
import math

import numpy as np
import pytest
import torch

from mapf_gpt_amd import training, weights
from tests import train_ref


def ref_lr(it, learning_rate=6e-4, warmup_iters=2000, lr_decay_iters=30000, min_lr=6e-5):
    if it < warmup_iters:
        return learning_rate * it / warmup_iters
    if it > lr_decay_iters:
        return min_lr
    decay_ratio = (it - warmup_iters) / (lr_decay_iters - warmup_iters)
    coeff = 0.5 * (1.0 + math.cos(math.pi * decay_ratio))
    return min_lr + coeff * (learning_rate - min_lr)


def test_lr_schedule_matches_train_py():
    d = training.DEFAULTS
    assert (d["learning_rate"], d["warmup_iters"], d["lr_decay_iters"], d["min_lr"]) == (6e-4, 2000, 30000, 6e-5)   # train.py:46-56
    assert (d["gradient_accumulation_steps"], d["batch_size"], d["grad_clip"], d["weight_decay"]) == (16, 64, 1.0, 0.1)
    for it in (0, 1, 999, 1999, 2000, 2001, 9000, 15000, 29999, 30000, 30001, 45000):
        assert training.get_lr(it, 6e-4, 2000, 30000, 6e-5) == ref_lr(it), it
    assert training.get_lr(3, 1e-3, 2, 4, 1e-4) == ref_lr(3, 1e-3, 2, 4, 1e-4)


def _write_shard(pa, path, x, y):
    table = pa.table({"input_tensors": pa.array(list(x)), "gt_actions": pa.array(y)})
    with pa.OSFile(str(path), "wb") as sink:
        with pa.ipc.new_file(sink, table.schema) as w:
            w.write_table(table)


def test_batches_match_fast_data_loader(tmp_path):
    pa = pytest.importorskip("pyarrow")
    rng = np.random.Generator(np.random.PCG64(4))
    shards = []
    for k, n in enumerate((5, 3)):
        x = rng.integers(0, 67, (n, 256)).astype(np.int8)
        y = rng.integers(0, 5, n).astype(np.int8)
        _write_shard(pa, tmp_path / f"part_{k}.arrow", x, y)
        shards.append((x, y))
    # restatement: files in name order, forever; each file shuffled when loaded (one generator), targets -1 but position 255, batches of 2
    g = np.random.Generator(np.random.PCG64(7))
    want = []
    for _ in range(3):
        for x, y in shards:
            idx = g.permutation(len(x))
            xs, ys = x[idx], y[idx]
            t = np.full(xs.shape, -1, np.int64)
            t[:, -1] = ys
            want += [(xs[i:i + 2], t[i:i + 2]) for i in range(0, len(xs), 2)]
    it = iter(training.ArrowBatches(str(tmp_path), 2, seed=7))
    for wx, wt in want:
        gx, gt = next(it)
        assert np.array_equal(gx, wx) and np.array_equal(gt, wt)
        assert (gt[:, :-1] == -1).all() and gt.dtype == np.int64
    # one file given directly
    one = iter(training.ArrowBatches(str(tmp_path / "part_1.arrow"), 8, seed=0))
    x1, t1 = next(one)
    assert x1.shape == (3, 256) and sorted(t1[:, -1].tolist()) == sorted(shards[1][1].tolist())


@pytest.mark.parametrize("name", ["tiny", "2M", "6M", "85M", *train_ref.LOCALISERS])
def test_trained_like_recipe_reaches_its_regime(name):
    """Conditions on the INPUTS of tests/test_gpu_train.py's and test_gpu_train_bf16.py's trained-like cases, on the fp64 oracle alone:
    peaked attention, GELU tails, gains of both signs and near zero, and a reference that meets _check_grads' hard clause itself."""
    tokens, targets, sd, args = train_ref.trained_like_case(name)
    for l, (spread, tail) in enumerate(train_ref.regime(sd, args, tokens)):
        assert spread >= 8.0, f"{name} layer {l}: median per-query score spread {spread:.2f} nats"
        assert tail >= 0.01, f"{name} layer {l}: share of |a| > 3 is {tail:.4f}"
    gains = [k for k in sd if k.endswith(("ln_1.weight", "ln_2.weight", "ln_f.weight"))]
    assert len(gains) == 2 * args["n_layer"] + 1
    for k in gains:
        assert sd[k].min() < 0 and np.abs(sd[k]).min() < 0.05, k
    base = weights.synthetic_state_dict(args, seed=0)
    assert set(sd) == set(base) and all(sd[k].shape == base[k].shape and sd[k].dtype == np.float32 for k in base)
    assert sd["lm_head.weight"] is sd["transformer.wte.weight"]
    l64, g64 = train_ref.loss_and_grads(sd, args, tokens, targets, torch.float64)
    _, g32 = train_ref.loss_and_grads(sd, args, tokens, targets, torch.float32)
    assert math.isfinite(l64)
    for k, ref in g64.items():
        assert bool(torch.isfinite(ref).all()), k
        m = float(ref.abs().max())
        e32 = float((g32[k].double() - ref).abs().max())
        assert m > 0 and e32 <= 1e-4 * m, f"{name} {k}: fp32 autograd {e32:.3e}, max|g64| {m:.3e}"
