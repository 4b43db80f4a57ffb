"""Torch restatement of model.py's TRAINING-mode forward (dropout at :129/:175, :59/:66, :71, :88) with manual attention, so that the masks
can be the library's own: they come from mapf_gpt_amd.sampling.dropout_keep / dropout_scale, the host specification of the device masks.
With p = 0 it is train_ref.loss_and_grads' forward (tests/test_train_dropout_cpu.py pins that).  Test infrastructure only."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from mapf_gpt_amd import sampling

SITE_EMBED, SITE_ATTN, SITE_ATTN_PROJ, SITE_MLP_PROJ = 0, 1, 2, 3


def factor(seed, step, site, layer, p, row0, rows, args, device):
    """float32 tensor m * s of one site: [rows, n_head, 256, 256] for the attention probabilities, [rows, 256, C] elsewhere"""
    nh, C = args["n_head"], args["n_embd"]
    n = rows * (nh * 65536 if site == SITE_ATTN else 256 * C)
    first = row0 * (nh * 65536 if site == SITE_ATTN else 256 * C)
    keep = sampling.dropout_keep(seed, step, site, layer, np.arange(first, first + n, dtype=np.uint64), p)
    f = torch.as_tensor(keep.astype(np.float32) * sampling.dropout_scale(p), device=device)
    return f.view(rows, nh, 256, 256) if site == SITE_ATTN else f.view(rows, 256, C)


def _drop(x, f):
    """nn.Dropout with the mask given: the product in fp32 (torch's opmath), rounded to x's dtype (fp64 stays fp64)"""
    if f is None:
        return x
    if x.dtype == torch.float64:
        return x * f.double()
    return (x.float() * f).to(x.dtype)


def forward_loss(view, args, tokens, targets, p=0.0, seed=0, step=0, row0=0, sites=15):
    """mean cross-entropy (ignore_index = -1) of the training-mode forward; runs under the caller's autocast context"""
    idx = torch.as_tensor(np.asarray(tokens)).long().to(view["transformer.wte.weight"].device)
    B, T = idx.shape
    L, nh, C = args["n_layer"], args["n_head"], args["n_embd"]
    hs = C // nh

    def f(site, layer):
        on = p > 0 and (sites >> site) & 1 and sampling.dropout_threshold(p) > 0
        return factor(seed, step, site, layer, p, row0, B, args, idx.device) if on else None

    x = _drop(view["transformer.wte.weight"][idx] + view["transformer.wpe.weight"][:T], f(SITE_EMBED, 0))       # model.py:171-175
    for l in range(L):
        w = lambda k: view[f"transformer.h.{l}.{k}.weight"]
        qkv = F.linear(F.layer_norm(x, (C,), w("ln_1"), None, 1e-5), w("attn.c_attn"))
        q, k, v = (t.view(B, T, nh, hs).transpose(1, 2) for t in qkv.split(C, dim=2))
        att = F.softmax((q @ k.transpose(-2, -1)) * (1.0 / math.sqrt(hs)), dim=-1)                              # model.py:63-65
        y = (_drop(att, f(SITE_ATTN, l)) @ v).transpose(1, 2).contiguous().view(B, T, C)                         # model.py:66-68
        x = x + _drop(F.linear(y, w("attn.c_proj")), f(SITE_ATTN_PROJ, l))                                       # model.py:71, 102
        h = F.gelu(F.linear(F.layer_norm(x, (C,), w("ln_2"), None, 1e-5), w("mlp.c_fc")))
        x = x + _drop(F.linear(h, w("mlp.c_proj")), f(SITE_MLP_PROJ, l))                                         # model.py:87-88, 103
    logits = F.layer_norm(x, (C,), view["transformer.ln_f.weight"], None, 1e-5) @ view["lm_head.weight"].t()
    tg = torch.as_tensor(np.asarray(targets)).long().reshape(-1).to(idx.device)
    return F.cross_entropy(logits.float().reshape(-1, 67) if logits.dtype != torch.float64 else logits.reshape(-1, 67), tg, ignore_index=-1)


def loss_and_grads(sd, args, tokens, targets, p, seed, step, row0=0, sites=15, dtype=torch.float64, autocast=False, loss_scale=1.0,
                   micro=None, device="cpu"):
    """-> (mean cross-entropy, {name: grad float64 cpu}) of one call, or of the calls micro = [(tokens, targets, row0), ...] (the same
    seed and step, loss_scale each).  autocast: fp32 leaves under torch.autocast(bfloat16) on `device`."""
    if autocast:
        dtype = torch.float32
    lv = {k: torch.tensor(np.asarray(v), dtype=dtype, device=device, requires_grad=True) for k, v in sd.items() if k != "lm_head.weight"}
    view = dict(lv)
    view["lm_head.weight"] = lv["transformer.wte.weight"]
    losses = []
    for tk, tg, r0 in (micro or [(tokens, targets, row0)]):
        with torch.autocast(torch.device(device).type, dtype=torch.bfloat16, enabled=autocast):
            loss = forward_loss(view, args, tk, tg, p, seed, step, r0, sites)
        (loss * loss_scale).backward()
        losses.append(float(loss.detach()))
    return (losses if micro else losses[0]), {k: v.grad.detach().double().cpu() for k, v in lv.items()}
