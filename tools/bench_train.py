"""Device training step timings (mgpt_gpt_forward_backward, clip + AdamW) against the exact-fp32 forward(idx, targets) of the same rows, and,
as a yardstick only, torch fp32 eager autograd of an in-repo restatement of model.py (oracle/gpt_oracle.py's formulas) on the same GPU.

    python tools/bench_train.py [--shapes 6M:512,6M:2048,2M:4096,85M:512] [--precision f32,bf16] [--torch-rows 512] [--iters 3] [--warmup 1]
                                [--dropout P] [--lib PATH] [--call general|rows|ab] [--accum N]
    python tools/bench_train.py --grad-sync WORLD [--grad-sync-shapes 6M,85M] [--iters 5] [--warmup 2]

--lib PATH times another build of the library (a file `python -m mapf_gpt_amd.build --out` writes) in place of the in-tree one: the same
command runs in a fresh child process with MGPT_LIB_PATH set.
--precision f32,bf16 times both training precisions in one call (one JSON line per shape and precision).  Every line carries the counted
flops of the call (the products the model executes, 2 per multiply-add, backward = 2 x forward; the attention backward's recomputed S
excluded) and, for bf16, the bytes its kernels move to and from memory (count_bytes below: every tensor read or written once per kernel,
weights and L2 reuse not counted), with the achieved rate and the roofline bound against 2.5 PFLOP/s (bf16 MFMA) or 157 TFLOP/s (fp32) and
8 TB/s.  The bf16 torch yardstick is the same restatement under torch.autocast("cuda", torch.bfloat16), train.py's regime.

--dropout P times forward_backward of a dropout = P model in training mode (masks regenerated in the kernels, none stored) and gives the
torch yardstick the same p: nn.Dropout at model.py's three places and scaled_dot_product_attention's dropout_p, torch's own streams.

--grad-sync WORLD times the device side of the data-parallel gradient synchronisation on one GPU (mapf_gpt_amd/training.py: export_grads,
all_gather, reduce_grads): GPT.export_grads() and GPT.reduce_grads(gathered, 1 / WORLD) with a gathered array of WORLD rows of the size of the
rank's own buffer, each as the median over --iters windows of 20 back-to-back calls between HIP events.  One JSON line per shape: microseconds
per call and the fraction of 8 TB/s by counted bytes (export: read n and write n floats; reduce: read WORLD x n and write n, (WORLD + 1) 4 n
bytes).  The all_gather itself is not in it: it needs the other ranks.  Nothing else runs in that mode.

--call rows times GPT.forward_backward_rows (the last-position micro-step: the last layer, head and loss on token 255 only, no host wait) on
the same rows and labels in place of forward_backward; --call ab times both in one process, alternating general, rows, general, rows ...
call by call, and prints for each the median and the range of its --iters timed regions.  --accum N puts N back-to-back micro-steps in a
timed region (gradient accumulation: the general call waits for the stream once per micro-step, the rows call never).  In these modes a
line carries the micro-step timings only (no clip + AdamW, forward or torch yardstick).  The default, --call general, is unchanged.
With --dropout P the rows call is GPT.forward_backward_rows_drop and the general call runs with the same p: --call ab --dropout 0.1 times
the two dropout micro-steps against each other on the same rows.

Targets follow the dataset's pattern (-1 except the last position, fast_data_loader.py:58).  Prints one JSON line per shape: median ms of
each part over --iters timed calls after --warmup untimed ones, HIP events on the current stream.  The torch yardstick runs on
min(rows, --torch-rows) rows (its activations are several times ours; 0 skips it) and reports the rows it ran."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mapf_gpt_amd.model import build_model  # noqa: E402


def timed_ab(fns, iters, warmup):
    """{name: [ms per timed region]} of the calls fns = {name: fn}, alternating between them region by region"""
    out = {k: [] for k in fns}
    for i in range(warmup + iters):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= warmup:
                out[k].append(a.elapsed_time(b))
    return out


def count_flops_rows(args, rows, T=256, V=67):
    """... of one forward_backward_rows call: the last layer keeps its K | V projection on all tokens (4 C^2 per token) and runs the rest,
    the head included, on one token per row"""
    C, L = args["n_embd"], args["n_layer"]
    return 3 * rows * (T * ((L - 1) * (24 * C * C + 4 * T * C) + 4 * C * C) + 20 * C * C + 4 * T * C + 2 * C * V)


def micro_steps(a, name, rows, args, tokens, targets):
    """--call rows / ab: the micro-step alone, a.accum of them per timed region"""
    labels = targets[:, -1].contiguous()
    for prec in a.precision.split(","):
        net = build_model(dict(args, dropout=a.dropout), seed=0, max_rows=rows)
        net.set_dropout_rng(0)
        net.train()

        def general():
            for _ in range(a.accum):
                net.forward_backward(tokens, targets, loss_scale=1.0 / a.accum, precision=prec)

        def rows_call():                        # (--dropout P: the call with the general call's masks, forward_backward_rows_drop)
            for _ in range(a.accum):
                if a.dropout > 0:
                    net.forward_backward_rows_drop(tokens, labels, loss_scale=1.0 / a.accum, precision=prec, check=False)
                else:
                    net.forward_backward_rows(tokens, labels, loss_scale=1.0 / a.accum, precision=prec, check=False)
        fns = {"general": general, "rows": rows_call} if a.call == "ab" else {"rows": rows_call}
        ms = timed_ab(fns, a.iters, a.warmup)
        rec = {"shape": name, "rows": rows, "precision": prec, "call": a.call, "accum": a.accum, "dropout": a.dropout}
        for k, v in ms.items():
            rec[k + "_ms"] = round(float(np.median(v)), 3)
            rec[k + "_range_ms"] = [round(min(v), 3), round(max(v), 3)]
        if a.call == "ab":
            rec["rows_over_general"] = round(rec["rows_ms"] / rec["general_ms"], 4)
            rec["ranges_overlap"] = not (max(ms["rows"]) < min(ms["general"]) or max(ms["general"]) < min(ms["rows"]))
            rec["flops_rows_over_general"] = round(count_flops_rows(args, rows) / count_flops(args, rows), 4)
        print(json.dumps(rec), flush=True)
        del net
        torch.cuda.empty_cache()


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


PEAK_FLOPS = {"f32": 157e12, "bf16": 2.5e15}
PEAK_BYTES = 8e12


def count_flops(args, rows, T=256, V=67):
    """products of one forward_backward call: per token and layer 24 C^2 (the four linears) + 4 T C (QK^T and PV), the head 2 C V;
    backward twice the forward"""
    C, L = args["n_embd"], args["n_layer"]
    return 3 * rows * T * (L * (24 * C * C + 4 * T * C) + 2 * C * V)


def count_bytes(args, rows, T=256, V=67):
    """bytes the bf16 path's kernels read and write per call (train.hip, the bf16 bodies of Chunk), per token and layer in units of C:
    forward 96 C (LayerNorms 2 x 8, q|k|v 16, attention 16, c_proj 12, c_fc 20 (bf16 a and gelu(a)), mlp c_proj 16);
    backward 200 C (d h with gelu' 20, the four weight gradients 12 + 12 + 8 + 16, the input gradients 12 + 8 + 16, LayerNorms 2 x 16,
    attention backward 64); the head and the embedding 16 V + 24 C per token"""
    C, L = args["n_embd"], args["n_layer"]
    return rows * T * (L * 296 * C + 16 * V + 24 * C)


def dropout_forward(w, args, idx, p):
    """model.py's training-mode forward up to the last block's output: oracle/gpt_oracle.py's formulas with dropout at :175, :59, :71, :88"""
    import torch.nn.functional as F
    B, T = idx.shape
    nh, C = args["n_head"], args["n_embd"]
    x = F.dropout(w["transformer.wte.weight"][idx] + w["transformer.wpe.weight"][:T], p)
    for l in range(args["n_layer"]):
        k_ = f"transformer.h.{l}."
        qkv = F.linear(F.layer_norm(x, (C,), w[k_ + "ln_1.weight"], None, 1e-5), w[k_ + "attn.c_attn.weight"])
        q, k, v = (t.view(B, T, nh, C // nh).transpose(1, 2) for t in qkv.split(C, dim=2))
        y = F.scaled_dot_product_attention(q, k, v, attn_mask=None, dropout_p=p, is_causal=False).transpose(1, 2).contiguous().view(B, T, C)
        x = x + F.dropout(F.linear(y, w[k_ + "attn.c_proj.weight"]), p)
        h = F.gelu(F.linear(F.layer_norm(x, (C,), w[k_ + "ln_2.weight"], None, 1e-5), w[k_ + "mlp.c_fc.weight"]))
        x = x + F.dropout(F.linear(h, w[k_ + "mlp.c_proj.weight"]), p)
    return x


def torch_step(name, tokens, targets, autocast=False, dropout=0.0):
    """torch fp32 eager (autocast: under torch.autocast("cuda", torch.bfloat16)): loss = cross-entropy of ln_f(x) @ wte^T over every
    position (model.py:178-184), backward into .grad; dropout > 0: the training-mode forward with torch's own masks"""
    import torch.nn.functional as F
    from mapf_gpt_amd import weights
    from oracle import gpt_oracle
    args = weights.model_args(name)
    sd = {k: torch.tensor(v, device="cuda", requires_grad=True) for k, v in weights.synthetic_state_dict(name, seed=0).items()
          if k != "lm_head.weight"}
    view = dict(sd)
    view["lm_head.weight"] = sd["transformer.wte.weight"]
    idx, tg = tokens.long(), targets.long()

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            x = dropout_forward(view, args, idx, dropout) if dropout > 0 else gpt_oracle.forward_logits(view, args, idx, return_layers=True)[1][-1]
            h = F.layer_norm(x, (x.shape[-1],), view["transformer.ln_f.weight"], None, 1e-5)
            loss = F.cross_entropy((h @ view["lm_head.weight"].t()).reshape(-1, 67), tg.reshape(-1), ignore_index=-1)
        loss.backward()
    return step


def grad_sync(world, shapes, iters, warmup, reps=20):
    """export_grads and reduce_grads of every shape: microseconds per call and the fraction of PEAK_BYTES by counted bytes"""
    for name in shapes:
        net = build_model(name, seed=0, max_rows=1).train()
        n = net.grads_size()
        flat = torch.empty(n, dtype=torch.float32, device="cuda")
        gathered = torch.randn((world, n), dtype=torch.float32, device="cuda")

        def export():
            for _ in range(reps):
                net.export_grads(flat)

        def reduce():
            for _ in range(reps):
                net.reduce_grads(gathered, 1.0 / world)
        ex, rd = timed(export, iters, warmup) / reps * 1e3, timed(reduce, iters, warmup) / reps * 1e3
        ex_bytes, rd_bytes = 2 * 4 * n, (world + 1) * 4 * n
        print(json.dumps({"shape": name, "grad_sync_world": world, "n_elem": n, "buffer_mb": round(4 * n / 1e6, 1),
                          "export_us": round(ex, 1), "export_frac_of_8TBps": round(ex_bytes / (ex * 1e-6) / PEAK_BYTES, 3),
                          "reduce_us": round(rd, 1), "reduce_mb": round(rd_bytes / 1e6, 1),
                          "reduce_frac_of_8TBps": round(rd_bytes / (rd * 1e-6) / PEAK_BYTES, 3),
                          "received_mb_per_rank": round((world - 1) * 4 * n / 1e6, 1)}), flush=True)
        del net, flat, gathered
        torch.cuda.empty_cache()


def main(argv=None):
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--lib", default=None)
    lib, rest = pre.parse_known_args(argv)
    if lib.lib:                 # mapf_gpt_amd/_lib.py reads the variable when it is imported, which has happened above
        return subprocess.run([sys.executable, os.path.abspath(__file__), *rest],
                              env=dict(os.environ, MGPT_LIB_PATH=os.path.abspath(lib.lib))).returncode
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="6M:512,6M:2048,2M:4096,85M:512")
    ap.add_argument("--precision", default="f32,bf16", help="comma-separated training precisions: f32, bf16")
    ap.add_argument("--torch-rows", type=int, default=512)
    ap.add_argument("--dropout", type=float, default=0.0, help="dropout probability of the timed call and of the torch yardstick")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--lib", default=None, help="path of the library to time (default: the in-tree build)")
    ap.add_argument("--call", default="general", choices=["general", "rows", "ab"],
                    help="general: forward_backward (default); rows: forward_backward_rows; ab: both, alternating in one process")
    ap.add_argument("--accum", type=int, default=1, help="--call rows / ab: back-to-back micro-steps per timed region")
    ap.add_argument("--grad-sync", type=int, default=0, metavar="WORLD",
                    help="time export_grads and reduce_grads over WORLD gathered buffers instead of the training step")
    ap.add_argument("--grad-sync-shapes", default="6M,85M")
    a = ap.parse_args(argv)
    if a.grad_sync > 0:
        return grad_sync(a.grad_sync, a.grad_sync_shapes.split(","), a.iters, a.warmup)
    for item in a.shapes.split(","):
        name, rows = item.split(":")
        rows = int(rows)
        rng = np.random.Generator(np.random.PCG64(0))
        tokens = torch.as_tensor(rng.integers(0, 67, (rows, 256)), dtype=torch.uint8).cuda()
        targets = torch.full((rows, 256), -1, dtype=torch.int32, device="cuda")
        targets[:, -1] = torch.as_tensor(rng.integers(0, 5, rows), dtype=torch.int32).cuda()
        from mapf_gpt_amd import weights
        args = weights.model_args(name)
        if a.call != "general":
            micro_steps(a, name, rows, args, tokens, targets)
            continue
        for prec in a.precision.split(","):
            net = build_model(dict(args, dropout=a.dropout), seed=0, max_rows=rows)
            net.set_dropout_rng(0)
            net.train()
            opt = net.configure_optimizers(0.1, 6e-4, (0.9, 0.95))
            fb = timed(lambda: net.forward_backward(tokens, targets, precision=prec), a.iters, a.warmup)

            def clip_step():
                net.clip_grad_norm_(1.0)
                opt.step()
            cs = timed(clip_step, a.iters, a.warmup)
            fw = timed(lambda: net.forward(tokens, targets), a.iters, a.warmup)
            flops = count_flops(args, rows)
            rec = {"shape": name, "rows": rows, "precision": prec, "dropout": a.dropout, "forward_backward_ms": round(fb, 3), "clip_step_ms": round(cs, 3),
                   "forward_f32_ms": round(fw, 3), "fb_over_forward": round(fb / fw, 3), "gflop": round(flops / 1e9, 1),
                   "tflops": round(flops / fb / 1e9, 1), "flop_bound_ms": round(flops / PEAK_FLOPS[prec] * 1e3, 3)}
            if prec == "bf16":
                nbytes = count_bytes(args, rows)
                rec.update({"gbytes": round(nbytes / 1e9, 2), "tbytes_per_s": round(nbytes / fb / 1e9, 2),
                            "byte_bound_ms": round(nbytes / PEAK_BYTES * 1e3, 3)})
            del net, opt
            torch.cuda.empty_cache()
            tr = min(rows, a.torch_rows)
            if tr > 0:
                rec["torch_rows"] = tr
                try:
                    key = "torch_autocast_fwd_bwd_ms" if prec == "bf16" else "torch_fwd_bwd_ms"
                    rec[key] = round(timed(torch_step(name, tokens[:tr], targets[:tr], prec == "bf16", a.dropout), a.iters, a.warmup), 3)
                    rec["ours_per_row_over_torch"] = round((fb / rows) / (rec[key] / tr), 3)
                except torch.cuda.OutOfMemoryError:
                    rec[key] = "out of memory"
                torch.cuda.empty_cache()
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    sys.exit(main())
