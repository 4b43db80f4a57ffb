"""fp64 restatement of the last-position micro-step (GPT.forward_backward_rows, csrc/train.hip: layer_forward_last / layer_backward_last):
the last layer on the compact matrix of the rows' last tokens with a HAND-WRITTEN backward -- the formulas the kernels implement, no
autograd through the last layer, ln_f, the head or the loss.  The layers below it and the embedding are the pinned oracle's under autograd
and receive the hand-computed gradient of the last layer's input.  Test infrastructure only."""
import math

import numpy as np
import torch

from oracle import gpt_oracle
from tests.train_ref import leaves


def _ln(x, w):
    """LayerNorm (eps 1e-5, gain only) -> (output, xhat, rstd)"""
    mean = x.mean(-1, keepdim=True)
    rstd = ((x - mean).pow(2).mean(-1, keepdim=True) + 1e-5).rsqrt()
    xhat = (x - mean) * rstd
    return xhat * w, xhat, rstd


def _ln_bwd(dy, w, xhat, rstd):
    """-> (d x, d gain): d x = rstd (g - mean(g) - xhat mean(g xhat)), g = dy w;  d gain = sum over the tokens of dy xhat"""
    g = dy * w
    dx = rstd * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
    return dx, (dy * xhat).reshape(-1, dy.shape[-1]).sum(0)


def _gelu(a):
    return 0.5 * a * (1.0 + torch.erf(a / math.sqrt(2.0)))


def _gelu_grad(a):
    return 0.5 * (1.0 + torch.erf(a / math.sqrt(2.0))) + a * torch.exp(-0.5 * a * a) / math.sqrt(2.0 * math.pi)


def last_layer_fwd_bwd(w, args, x, labels, n_rows, loss_scale=1.0):
    """x [B, 256, C]: the last layer's input (no graph).  -> (mean loss over the B rows, d x [B, 256, C], {name: grad} of the last layer,
    ln_f and the tied head).  The normaliser is n_rows (the whole call's rows)."""
    B, T, C = x.shape
    nh = args["n_head"]
    hs, scale = C // nh, 1.0 / math.sqrt(C // nh)
    p_ = f"transformer.h.{args['n_layer'] - 1}."
    Wq, Wk, Wv = w[p_ + "attn.c_attn.weight"].split(C, dim=0)
    Wp, Wfc, Wp2, wte = w[p_ + "attn.c_proj.weight"], w[p_ + "mlp.c_fc.weight"], w[p_ + "mlp.c_proj.weight"], w["transformer.wte.weight"]
    g1, g2, gf = w[p_ + "ln_1.weight"], w[p_ + "ln_2.weight"], w["transformer.ln_f.weight"]
    # forward: ln_1 and K | V on all tokens, everything else on token 255
    xn1, xh1, r1 = _ln(x, g1)
    K, V = (xn1 @ Wk.t()).view(B, T, nh, hs), (xn1 @ Wv.t()).view(B, T, nh, hs)
    xc, xn1c = x[:, -1], xn1[:, -1]
    q = (xn1c @ Wq.t()).view(B, nh, hs)
    s = torch.einsum("bhd,bjhd->bhj", q, K) * scale
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    p = e / e.sum(-1, keepdim=True)                                  # [B, nh, 256]
    y = torch.einsum("bhj,bjhd->bhd", p, V).reshape(B, C)
    xm = xc + y @ Wp.t()
    xn2, xh2, r2 = _ln(xm, g2)
    a = xn2 @ Wfc.t()
    h = _gelu(a)
    xo = xm + h @ Wp2.t()
    xnf, xhf, rf = _ln(xo, gf)
    logits = xnf @ wte.t()
    lse = torch.logsumexp(logits, -1)
    lb = torch.as_tensor(np.asarray(labels)).long()
    loss = (lse - logits[torch.arange(B), lb]).sum() / n_rows
    # backward
    grads = {}
    dlog = torch.exp(logits - lse[:, None])
    dlog[torch.arange(B), lb] -= 1.0
    dlog *= loss_scale / n_rows
    grads["transformer.wte.weight"] = dlog.t() @ xnf
    dxo, grads["transformer.ln_f.weight"] = _ln_bwd(dlog @ wte, gf, xhf, rf)
    grads[p_ + "mlp.c_proj.weight"] = dxo.t() @ h
    da = (dxo @ Wp2) * _gelu_grad(a)
    grads[p_ + "mlp.c_fc.weight"] = da.t() @ xn2
    d, grads[p_ + "ln_2.weight"] = _ln_bwd(da @ Wfc, g2, xh2, r2)
    dxm = dxo + d
    grads[p_ + "attn.c_proj.weight"] = dxm.t() @ y
    dy = (dxm @ Wp).view(B, nh, hs)
    D = (dy * y.view(B, nh, hs)).sum(-1, keepdim=True)              # [B, nh, 1]
    dp = torch.einsum("bhd,bjhd->bhj", dy, V)
    ds = p * (dp - D)
    dq = scale * torch.einsum("bhj,bjhd->bhd", ds, K).reshape(B, C)
    dK = scale * torch.einsum("bhj,bhd->bjhd", ds, q).reshape(B, T, C)
    dV = torch.einsum("bhj,bhd->bjhd", p, dy).reshape(B, T, C)
    dxn1 = dK @ Wk + dV @ Wv
    dxn1[:, -1] += dq @ Wq
    flat = xn1.reshape(B * T, C)
    grads[p_ + "attn.c_attn.weight"] = torch.cat([dq.t() @ xn1c, dK.reshape(B * T, C).t() @ flat, dV.reshape(B * T, C).t() @ flat])
    dx, grads[p_ + "ln_1.weight"] = _ln_bwd(dxn1, g1, xh1, r1)
    dx[:, -1] += dxm
    return float(loss), dx, grads


def loss_and_grads_rows(sd, args, tokens, labels, loss_scale=1.0):
    """-> (mean cross-entropy of the rows' last positions, {name: grad}) in fp64: = tests.train_ref.loss_and_grads(sd, args, tokens,
    targets_last(labels)) up to rounding, by the compact route"""
    lv, view = leaves(sd, torch.float64)
    L = args["n_layer"]
    x_in = gpt_oracle.forward_logits(view, args, np.asarray(tokens), dtype=torch.float64, return_layers=True)[1][L - 1]
    with torch.no_grad():
        w = {k: v.detach() for k, v in lv.items()}
        loss, dx, hand = last_layer_fwd_bwd(w, args, x_in.detach(), labels, len(tokens), loss_scale)
    x_in.backward(dx)
    out = {}
    for k, v in lv.items():
        g = v.grad.detach().clone() if v.grad is not None else torch.zeros_like(v)
        out[k] = g + hand[k] if k in hand else g
    return loss, out
