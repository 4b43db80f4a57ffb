"""bf16 mixed-precision training with dropout (GPT.forward_backward(..., precision="bf16") of a config.dropout > 0 model).

The truth g64 is fp64 autograd of the masked restatement (tests/train_dropout_ref.py), the yardstick g_ac the same restatement with the
same masks on cuda leaves under torch.autocast("cuda", torch.bfloat16).  The bar is tests/test_gpu_train_bf16.py's: for every tensor
max|g - g64| <= 2 max|g_ac - g64| + 1e-3 max|g64|, and |l - l64| <= 2 |l_ac - l64| + 2e-3 |l64| for the loss."""
import functools

import pytest
import torch

from tests import train_dropout_ref as ref
from tests.test_gpu_train import _dev_grads
from tests.test_gpu_train_bf16 import _check, _kernel_report
from tests.test_gpu_train_dropout import SEED, STEP, _bits_equal, _case, _net
from tests.train_ref import LOCALISERS

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _reference(name, rows, case, p, sites=15):
    tokens, targets, sd, args = _case(name, rows, case)
    l64, g64 = ref.loss_and_grads(sd, args, tokens, targets, p, SEED, STEP, 0, sites, torch.float64, device="cuda")
    lac, gac = ref.loss_and_grads(sd, args, tokens, targets, p, SEED, STEP, 0, sites, autocast=True, device="cuda")
    return l64, g64, lac, gac


def _run(label, name, rows, case, p, sites=15, train_rows=None):
    net, tk, tg = _net(name, rows, case, p, train_rows=train_rows)
    net.zero_grad()
    loss = float(net.forward_backward(tk, tg, precision="bf16", dropout_step=STEP, dropout_sites=sites))
    got = _dev_grads(net)
    l64, g64, lac, gac = _reference(name, rows, case, p, sites)
    try:
        _check(label, got, g64, gac, loss, l64, lac)
    except AssertionError as e:
        if name in LOCALISERS:
            raise AssertionError(f"{e}\n{_kernel_report(label, got, g64, gac, net._args['n_embd'])}") from None
        raise
    return net, tk, tg, got


@pytest.mark.parametrize("case", ["last", "all"])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("name", ["tiny", "1x2x64", "1x4x256", "2M", "6M"])
def test_bf16_dropout_gradients_within_the_autocast_bar(name, p, case):
    _run(f"bf16 dropout {name} p={p} {case}", name, 2 if name == "6M" else 3, case, p)


@pytest.mark.parametrize("sites", [1, 2, 4, 8])
@pytest.mark.parametrize("name", list(LOCALISERS))
def test_bf16_one_site_at_a_time(name, sites):
    _run(f"bf16 dropout {name} sites={sites}", name, 2, "all", 0.5, sites)


def test_bf16_chunked_call_and_bit_reproducibility():
    net, tk, tg, got = _run("bf16 dropout chunked", "tiny", 3, "all", 0.5, train_rows=2)
    net.zero_grad()
    net.forward_backward(tk, tg, precision="bf16", dropout_step=STEP)
    assert _bits_equal(_dev_grads(net), got), "two identical bf16 calls differ"
    net.zero_grad()
    net.forward_backward(tk, tg, precision="bf16", dropout_step=STEP + 1)
    assert not _bits_equal(_dev_grads(net), got)
