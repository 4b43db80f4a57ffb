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


# ----- a trained-like checkpoint: peaked attention, GELU tails, LayerNorm gains of both signs, a head far from uniform -----
# (n_layer, n_head, n_embd) -> (q/k factor, c_fc factor).  At N(0, 0.02) the scores spread by ~0.1 nat and no c_fc pre-activation reaches
# |a| = 3; these factors, tuned on the fp64 oracle alone (tests/test_train_cpu.py pins them), put every layer at a median per-query score
# spread >= 8 nats and >= 1 % of the pre-activations beyond |a| = 3.
TRAINED_LIKE = {
    (2, 2, 64): (16.0, 12.0),      # tiny
    (5, 5, 160): (7.0, 6.0),       # 2M
    (8, 8, 256): (7.0, 6.0),       # 6M
    (12, 12, 768): (4.0, 6.0),     # 85M
    (1, 2, 64): (16.0, 12.0),      # one layer, head size 32
    (1, 4, 256): (7.0, 6.0),       # one layer, head size 64
}
WTE_FACTOR = 4.0
# one-layer models that name a kernel rather than a model when they fail: head size 32 and head size 64
LOCALISERS = {"1x2x64": dict(n_layer=1, n_head=2, n_embd=64), "1x4x256": dict(n_layer=1, n_head=4, n_embd=256)}


def trained_like_state_dict(name_or_args, seed=0):
    """synthetic_state_dict with the q and k rows of every c_attn.weight and every c_fc.weight multiplied by the shape's factors, wte (the
    tied head) by WTE_FACTOR, and every LayerNorm gain redrawn from N(0, 1) with two entries set inside (-0.05, 0.05) and one made negative."""
    from mapf_gpt_amd import weights
    a = weights.model_args(name_or_args)
    L, C = a["n_layer"], a["n_embd"]
    fqk, ffc = TRAINED_LIKE[(L, a["n_head"], C)]
    sd = {k: np.array(v, dtype=np.float32) for k, v in weights.synthetic_state_dict(a, seed=seed).items()}
    rng = np.random.Generator(np.random.PCG64([seed, 0x7261696e]))

    def gain():
        g = rng.standard_normal(C)
        i = rng.permutation(C)[:3]
        g[i[0]], g[i[1]] = 0.03 * rng.random(), -0.03 * rng.random()
        g[i[2]] = -abs(g[i[2]]) - 0.1
        return g.astype(np.float32)

    for l in range(L):
        p = f"transformer.h.{l}."
        sd[p + "attn.c_attn.weight"][:2 * C] *= np.float32(fqk)
        sd[p + "mlp.c_fc.weight"] *= np.float32(ffc)
        sd[p + "ln_1.weight"], sd[p + "ln_2.weight"] = gain(), gain()
    sd["transformer.ln_f.weight"] = gain()
    sd["transformer.wte.weight"] *= np.float32(WTE_FACTOR)
    sd["lm_head.weight"] = sd["transformer.wte.weight"]
    return sd


def regime(sd, args, tokens):
    """fp64, per layer: (median over the queries of every row and head of max - min score, share of c_fc pre-activations with |a| > 3)"""
    import torch.nn.functional as F
    from oracle import gpt_oracle
    xs = gpt_oracle.forward_logits(sd, args, np.asarray(tokens), dtype=torch.float64, return_layers=True)[1]
    w = gpt_oracle.to_torch(sd, torch.float64)
    nh, C = args["n_head"], args["n_embd"]
    out = []
    for l in range(args["n_layer"]):
        p, x = f"transformer.h.{l}.", xs[l]
        B, T, _ = x.shape
        qkv = F.linear(F.layer_norm(x, (C,), w[p + "ln_1.weight"], None, 1e-5), w[p + "attn.c_attn.weight"])
        q, k, v = (t.view(B, T, nh, C // nh).transpose(1, 2) for t in qkv.split(C, dim=2))
        s = q @ k.transpose(-1, -2) / (C // nh) ** 0.5
        spread = float((s.max(-1).values - s.min(-1).values).median())
        y = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, T, C)
        xm = x + F.linear(y, w[p + "attn.c_proj.weight"])
        a = F.linear(F.layer_norm(xm, (C,), w[p + "ln_2.weight"], None, 1e-5), w[p + "mlp.c_fc.weight"])
        out.append((spread, float((a.abs() > 3).double().mean())))
    return out


def expert_rows(n, seed=0):
    """expert rows of the committed dataset fixtures (inputs / gt_actions of the reference's tokenizer)"""
    import os
    from tests.helpers import GOLDEN
    a, b = np.load(os.path.join(GOLDEN, "ds_random.npz")), np.load(os.path.join(GOLDEN, "ds_maze.npz"))
    x = np.concatenate([a["inputs"], b["inputs"]]).astype(np.int64)
    y = np.concatenate([a["gt_actions"], b["gt_actions"]]).astype(np.int64)
    idx = np.random.Generator(np.random.PCG64(seed)).permutation(len(x))[:n]
    return x[idx], y[idx]


def targets_mixed(rows, seed=1):
    """about half the positions targeted with a random vocabulary id, row 1 with no targeted position"""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = rng.integers(0, 67, (rows, 256)).astype(np.int64)
    t[rng.random((rows, 256)) < 0.5] = -1
    t[1] = -1
    return t


def trained_like_case(name, rows=None, seed=0):
    """-> (tokens, "mixed" targets, state dict, model args) of a trained-like gradient case: 3 rows (85M: 2) unless given"""
    from mapf_gpt_amd import weights
    args = weights.model_args(LOCALISERS.get(name, name))
    rows = rows or (2 if name == "85M" else 3)
    tokens, _ = expert_rows(rows, seed=len(name))
    return tokens, targets_mixed(rows), trained_like_state_dict(args, seed), args
