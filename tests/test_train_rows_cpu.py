"""The last-position micro-step without a GPU: the math its kernels implement (tests/train_rows_ref.py: the compact last layer with a
hand-written backward) against fp64 autograd of the general restatement on last-only targets, ArrowBatches(labels=True) against the
default mode, and the --rows-call flag of the training CLI."""
import os

import numpy as np
import pytest
import torch

from mapf_gpt_amd import training, weights
from mapf_gpt_amd.dataset_build import write_arrow
from tests.train_ref import LOCALISERS, expert_rows, loss_and_grads, targets_last, trained_like_state_dict
from tests.train_rows_ref import loss_and_grads_rows


@pytest.mark.parametrize("trained", [False, True], ids=["synthetic", "trained-like"])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("name", ["tiny", *LOCALISERS])
def test_compact_last_layer_matches_fp64_autograd(name, rows, trained):
    """both sides fp64, differing by rounding only: the loss and every gradient within 1e-9 max|g|"""
    args = weights.model_args(LOCALISERS.get(name, name))
    sd = trained_like_state_dict(args) if trained else weights.synthetic_state_dict(args, seed=0)
    tokens, labels = expert_rows(rows, seed=len(name))
    l_ref, g_ref = loss_and_grads(sd, args, tokens, targets_last(labels), torch.float64)
    loss, got = loss_and_grads_rows(sd, args, tokens, labels)
    assert abs(loss - l_ref) <= 1e-9 * abs(l_ref), (loss, l_ref)
    assert set(got) == set(g_ref)
    for k, ref in g_ref.items():
        m = float(ref.abs().max())
        err = float((got[k] - ref).abs().max())
        assert err <= 1e-9 * m, f"{name} {k}: max|g - g64| {err:.3e}, max|g64| {m:.3e}"


def test_compact_last_layer_loss_scale():
    args = weights.model_args("tiny")
    sd = weights.synthetic_state_dict(args, seed=0)
    tokens, labels = expert_rows(3, seed=4)
    _, g_ref = loss_and_grads(sd, args, tokens, targets_last(labels), torch.float64, loss_scale=0.5)
    _, got = loss_and_grads_rows(sd, args, tokens, labels, loss_scale=0.5)
    for k, ref in g_ref.items():
        assert float((got[k] - ref).abs().max()) <= 1e-9 * float(ref.abs().max()), k


def _shards(d, counts=(10, 7), bad=None):
    tokens, labels = expert_rows(sum(counts), seed=5)
    labels = np.array(labels, np.int64)
    if bad is not None:
        labels[counts[0] + 2] = bad                       # (in the second file)
    at = 0
    for i, n in enumerate(counts):
        write_arrow(os.path.join(d, f"part_{i}.arrow"), tokens[at:at + n].astype(np.int8), labels[at:at + n])
        at += n


def test_arrow_batches_labels_mode_matches_default(tmp_path):
    pytest.importorskip("pyarrow")
    _shards(str(tmp_path))
    default = iter(training.ArrowBatches(str(tmp_path), 4, seed=7))
    compact = iter(training.ArrowBatches(str(tmp_path), 4, seed=7, labels=True))
    for _ in range(2 * (3 + 2)):                          # two passes over the two files: batches of 4, 4, 2 and 4, 3
        (x, t), (xl, y) = next(default), next(compact)
        assert np.array_equal(x, xl) and y.shape == (len(x),) and y.dtype == np.int64
        assert np.array_equal(t[:, -1], y) and (t[:, :-1] == -1).all()


@pytest.mark.parametrize("bad", [67, -1])
def test_arrow_batches_labels_mode_validates_at_load(tmp_path, bad):
    pytest.importorskip("pyarrow")
    _shards(str(tmp_path), bad=bad)
    it = iter(training.ArrowBatches(str(tmp_path), 4, seed=7, labels=True))
    for _ in range(3):                                    # the first file is fine
        next(it)
    with pytest.raises(ValueError, match="labels must lie"):
        next(it)
    default = iter(training.ArrowBatches(str(tmp_path), 4, seed=7))      # the default mode is as it was: no check
    for _ in range(5):
        next(default)


def test_rows_call_flag():
    base = ["--init", "tiny", "--data", "d", "--val", "v"]
    assert training.parse_args(base).rows_call is False
    assert training.parse_args(base + ["--rows-call"]).rows_call is True
    assert training.parse_args(base + ["--rows-call", "--dropout", "0"]).rows_call is True
    with pytest.raises(SystemExit):
        training.parse_args(base + ["--rows-call", "--dropout", "0.1"])
    assert training.parse_args(base + ["--dropout", "0.1"]).dropout == 0.1
