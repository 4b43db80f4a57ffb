"""fp64 restatement of the last-position micro-step WITH dropout (GPT.forward_backward_rows_drop, csrc/train.hip: layer_forward_last /
layer_backward_last under a DropCfg): the compact last layer with the masks of the general call at token / query 255 and a HAND-WRITTEN
backward -- the formulas the kernels implement.  Autograd runs only below the last layer, on the masked embedding and the masked dense
layers 0 .. L-2 (tests.train_dropout_ref's masks and rounding).  The compact mask indices are computed here as the kernels compute them:
  site 1     ((row0 + row) n_head + head) 65536 + 255 * 256 + key
  sites 2, 3 ((row0 + row) 256 + 255) C + c          (the mask's row pitch is 256 C, the compact matrix's C)
Test infrastructure only."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from mapf_gpt_amd import sampling
from tests import train_dropout_ref as tdr
from tests.train_ref import leaves
from tests.train_rows_ref import _gelu, _gelu_grad, _ln, _ln_bwd

T = 256


def compact_index(site, args, row0, rows):
    """element indices of the compact last layer's masks: [rows, n_head, 256] (site 1: query 255, every key) or [rows, C] (sites 2, 3)"""
    nh, C = args["n_head"], args["n_embd"]
    r = (np.uint64(row0) + np.arange(rows, dtype=np.uint64))
    if site == tdr.SITE_ATTN:
        bh = r[:, None] * np.uint64(nh) + np.arange(nh, dtype=np.uint64)[None, :]
        return bh[:, :, None] * np.uint64(65536) + np.uint64((T - 1) * T) + np.arange(T, dtype=np.uint64)[None, None, :]
    return (r[:, None] * np.uint64(T) + np.uint64(T - 1)) * np.uint64(C) + np.arange(C, dtype=np.uint64)[None, :]


def compact_factor(seed, step, site, layer, p, row0, rows, args):
    """float64 tensor m * s of one site of the compact last layer (s the float32 factor of the device)"""
    keep = sampling.dropout_keep(seed, step, site, layer, compact_index(site, args, row0, rows), p)
    return torch.as_tensor(keep.astype(np.float64) * float(sampling.dropout_scale(p)))


def lower_layers(view, args, tokens, p, seed, step, row0, sites):
    """the input of the last layer, [B, 256, C] with its graph: the masked embedding and the masked layers 0 .. L-2 (train_dropout_ref's
    forward, stopped before the last layer)"""
    idx = torch.as_tensor(np.asarray(tokens)).long()
    B = idx.shape[0]
    L, nh, C = args["n_layer"], args["n_head"], args["n_embd"]
    hs = C // nh

    def f(site, layer):
        on = p > 0 and (sites >> site) & 1 and sampling.dropout_threshold(p) > 0
        return tdr.factor(seed, step, site, layer, p, row0, B, args, idx.device) if on else None

    x = tdr._drop(view["transformer.wte.weight"][idx] + view["transformer.wpe.weight"][:T], f(tdr.SITE_EMBED, 0))
    for l in range(L - 1):
        w = lambda k: view[f"transformer.h.{l}.{k}.weight"]
        qkv = F.linear(F.layer_norm(x, (C,), w("ln_1"), None, 1e-5), w("attn.c_attn"))
        q, k, v = (t.view(B, T, nh, hs).transpose(1, 2) for t in qkv.split(C, dim=2))
        att = F.softmax((q @ k.transpose(-2, -1)) * (1.0 / math.sqrt(hs)), dim=-1)
        y = (tdr._drop(att, f(tdr.SITE_ATTN, l)) @ v).transpose(1, 2).contiguous().view(B, T, C)
        x = x + tdr._drop(F.linear(y, w("attn.c_proj")), f(tdr.SITE_ATTN_PROJ, l))
        h = F.gelu(F.linear(F.layer_norm(x, (C,), w("ln_2"), None, 1e-5), w("mlp.c_fc")))
        x = x + tdr._drop(F.linear(h, w("mlp.c_proj")), f(tdr.SITE_MLP_PROJ, l))
    return x


def last_layer_fwd_bwd_drop(w, args, x, labels, n_rows, f1, f2, f3, loss_scale=1.0):
    """tests.train_rows_ref.last_layer_fwd_bwd with masks: f1 [B, n_head, 256] (m s of the probabilities of query 255), f2, f3 [B, C]
    (m s of the two residual branches at token 255); None = that site is off.
    Forward: l sums over all keys, y = sum_j m_j s p_j v_j; x_mid = x + m s c_proj(y); x_out = x_mid + m s c_proj(gelu(..)).
    Backward: the gradient entering each c_proj is m s d x and d x passes on unmasked; dp_j = m_j s (dy . v_j), D = dy . y,
    ds_j = p_j (dp_j - D), dV_j = m_j s p_j dy."""
    B, _, C = x.shape
    nh = args["n_head"]
    hs, scale = C // nh, 1.0 / math.sqrt(C // nh)
    one = torch.ones((), dtype=x.dtype)
    f1, f2, f3 = (one if f is None else f.to(x.dtype) for f in (f1, f2, f3))
    p_ = f"transformer.h.{args['n_layer'] - 1}."
    Wq, Wk, Wv = w[p_ + "attn.c_attn.weight"].split(C, dim=0)
    Wp, Wfc, Wp2, wte = w[p_ + "attn.c_proj.weight"], w[p_ + "mlp.c_fc.weight"], w[p_ + "mlp.c_proj.weight"], w["transformer.wte.weight"]
    g1, g2, gf = w[p_ + "ln_1.weight"], w[p_ + "ln_2.weight"], w["transformer.ln_f.weight"]
    xn1, xh1, r1 = _ln(x, g1)
    K, V = (xn1 @ Wk.t()).view(B, T, nh, hs), (xn1 @ Wv.t()).view(B, T, nh, hs)
    xc, xn1c = x[:, -1], xn1[:, -1]
    q = (xn1c @ Wq.t()).view(B, nh, hs)
    s = torch.einsum("bhd,bjhd->bhj", q, K) * scale
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    p = e / e.sum(-1, keepdim=True)                                  # [B, nh, 256]: the sum runs over all keys, dropped ones included
    pm = p * f1
    y = torch.einsum("bhj,bjhd->bhd", pm, V).reshape(B, C)
    xm = xc + f2 * (y @ Wp.t())
    xn2, xh2, r2 = _ln(xm, g2)
    a = xn2 @ Wfc.t()
    h = _gelu(a)
    xo = xm + f3 * (h @ Wp2.t())
    xnf, xhf, rf = _ln(xo, gf)
    logits = xnf @ wte.t()
    lse = torch.logsumexp(logits, -1)
    lb = torch.as_tensor(np.asarray(labels)).long()
    loss = (lse - logits[torch.arange(B), lb]).sum() / n_rows
    grads = {}
    dlog = torch.exp(logits - lse[:, None])
    dlog[torch.arange(B), lb] -= 1.0
    dlog *= loss_scale / n_rows
    grads["transformer.wte.weight"] = dlog.t() @ xnf
    dxo, grads["transformer.ln_f.weight"] = _ln_bwd(dlog @ wte, gf, xhf, rf)
    db = f3 * dxo                                                    # enters the MLP's c_proj; dxo itself passes on
    grads[p_ + "mlp.c_proj.weight"] = db.t() @ h
    da = (db @ Wp2) * _gelu_grad(a)
    grads[p_ + "mlp.c_fc.weight"] = da.t() @ xn2
    d, grads[p_ + "ln_2.weight"] = _ln_bwd(da @ Wfc, g2, xh2, r2)
    dxm = dxo + d
    db = f2 * dxm                                                    # enters attention's c_proj
    grads[p_ + "attn.c_proj.weight"] = db.t() @ y
    dy = (db @ Wp).view(B, nh, hs)
    D = (dy * y.view(B, nh, hs)).sum(-1, keepdim=True)
    dp = torch.einsum("bhd,bjhd->bhj", dy, V) * f1
    ds = p * (dp - D)
    dq = scale * torch.einsum("bhj,bjhd->bhd", ds, K).reshape(B, C)
    dK = scale * torch.einsum("bhj,bhd->bjhd", ds, q).reshape(B, T, C)
    dV = torch.einsum("bhj,bhd->bjhd", pm, dy).reshape(B, T, C)
    dxn1 = dK @ Wk + dV @ Wv
    dxn1[:, -1] += dq @ Wq
    flat = xn1.reshape(B * T, C)
    grads[p_ + "attn.c_attn.weight"] = torch.cat([dq.t() @ xn1c, dK.reshape(B * T, C).t() @ flat, dV.reshape(B * T, C).t() @ flat])
    dx, grads[p_ + "ln_1.weight"] = _ln_bwd(dxn1, g1, xh1, r1)
    dx[:, -1] += dxm
    return float(loss), dx, grads


def loss_and_grads_rows_drop(sd, args, tokens, labels, p, seed, step, row0=0, sites=15, loss_scale=1.0):
    """-> (mean cross-entropy of the rows' last positions, {name: grad}) in fp64: = tests.train_dropout_ref.loss_and_grads(sd, args, tokens,
    targets_last(labels), p, seed, step, row0, sites) up to rounding, by the compact route"""
    lv, view = leaves(sd, torch.float64)
    L, B = args["n_layer"], len(tokens)
    x_in = lower_layers(view, args, tokens, p, seed, step, row0, sites)

    def f(site):
        on = p > 0 and (sites >> site) & 1 and sampling.dropout_threshold(p) > 0
        return compact_factor(seed, step, site, L - 1, p, row0, B, args) if on else None

    with torch.no_grad():
        w = {k: v.detach() for k, v in lv.items()}
        loss, dx, hand = last_layer_fwd_bwd_drop(w, args, x_in.detach(), labels, B, f(tdr.SITE_ATTN), f(tdr.SITE_ATTN_PROJ),
                                                 f(tdr.SITE_MLP_PROJ), loss_scale)
    x_in.backward(dx)
    out = {}
    for k, v in lv.items():
        g = v.grad.detach().clone() if v.grad is not None else torch.zeros_like(v)
        out[k] = g + hand[k] if k in hand else g
    return loss, out
