"""Autograd restatement of train.py's micro-step on the pinned oracle's forward (oracle/gpt_oracle.py + ln_f / tied head / cross-entropy of
tests/test_loss_cpu.py): the yardstick of the device training path.  Test infrastructure only."""
import numpy as np
import torch

from tests.test_loss_cpu import seq_oracle


def leaves(sd, dtype):
    """Leaf tensors (requires_grad) by named_parameters name, and the state_dict view with lm_head.weight tied to transformer.wte.weight."""
    lv = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in sd.items() if k != "lm_head.weight"}
    view = dict(lv)
    view["lm_head.weight"] = lv["transformer.wte.weight"]
    return lv, view


def loss_and_grads(sd, args, tokens, targets, dtype=torch.float64, loss_scale=1.0, micro=None):
    """-> (mean cross-entropy, {name: grad}) of one micro-step (micro=None) or of the micro-steps [(tokens, targets), ...] with loss_scale each."""
    lv, view = leaves(sd, dtype)
    losses = []
    for tk, tg in (micro or [(tokens, targets)]):
        _, loss = seq_oracle(view, args, np.asarray(tk), torch.as_tensor(np.asarray(tg)), dtype=dtype)
        (loss * loss_scale).backward()
        losses.append(float(loss))
    return (losses if micro else losses[0]), {k: v.grad.detach().clone() for k, v in lv.items()}


def targets_last(actions, T=256):
    """fast_data_loader.py:58: -1 everywhere except the last position, which holds the expert action."""
    t = np.full((len(actions), T), -1, np.int64)
    t[:, -1] = np.asarray(actions, np.int64)
    return t
