"""Device training step timings (mgpt_gpt_forward_backward, clip + AdamW) against the exact-fp32 forward(idx, targets) of the same rows, and,
as a yardstick only, torch fp32 eager autograd of an in-repo restatement of model.py (oracle/gpt_oracle.py's formulas) on the same GPU.

    python tools/bench_train.py [--shapes 6M:512,6M:2048,2M:4096,85M:512] [--torch-rows 512] [--iters 3] [--warmup 1]

Targets follow the dataset's pattern (-1 except the last position, fast_data_loader.py:58).  Prints one JSON line per shape: median ms of
each part over --iters timed calls after --warmup untimed ones, HIP events on the current stream.  The torch yardstick runs on
min(rows, --torch-rows) rows (its activations are several times ours; 0 skips it) and reports the rows it ran."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mapf_gpt_amd.model import build_model  # noqa: E402


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


def torch_step(name, tokens, targets):
    """torch fp32 eager: loss = cross-entropy of ln_f(x) @ wte^T over every position (model.py:178-184), backward into .grad"""
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
        x = gpt_oracle.forward_logits(view, args, idx, return_layers=True)[1][-1]
        h = F.layer_norm(x, (x.shape[-1],), view["transformer.ln_f.weight"], None, 1e-5)
        loss = F.cross_entropy((h @ view["lm_head.weight"].t()).reshape(-1, 67), tg.reshape(-1), ignore_index=-1)
        loss.backward()
    return step


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="6M:512,6M:2048,2M:4096,85M:512")
    ap.add_argument("--torch-rows", type=int, default=512)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args(argv)
    for item in a.shapes.split(","):
        name, rows = item.split(":")
        rows = int(rows)
        rng = np.random.Generator(np.random.PCG64(0))
        tokens = torch.as_tensor(rng.integers(0, 67, (rows, 256)), dtype=torch.uint8).cuda()
        targets = torch.full((rows, 256), -1, dtype=torch.int32, device="cuda")
        targets[:, -1] = torch.as_tensor(rng.integers(0, 5, rows), dtype=torch.int32).cuda()
        net = build_model(name, seed=0, max_rows=rows).train()
        opt = net.configure_optimizers(0.1, 6e-4, (0.9, 0.95))
        fb = timed(lambda: net.forward_backward(tokens, targets), a.iters, a.warmup)

        def clip_step():
            net.clip_grad_norm_(1.0)
            opt.step()
        cs = timed(clip_step, a.iters, a.warmup)
        fw = timed(lambda: net.forward(tokens, targets), a.iters, a.warmup)
        rec = {"shape": name, "rows": rows, "forward_backward_ms": round(fb, 3), "clip_step_ms": round(cs, 3),
               "forward_f32_ms": round(fw, 3), "fb_over_forward": round(fb / fw, 3)}
        del net, opt
        torch.cuda.empty_cache()
        tr = min(rows, a.torch_rows)
        if tr > 0:
            rec["torch_rows"] = tr
            try:
                rec["torch_fwd_bwd_ms"] = round(timed(torch_step(name, tokens[:tr], targets[:tr]), a.iters, a.warmup), 3)
                rec["ours_per_row_over_torch"] = round((fb / rows) / (rec["torch_fwd_bwd_ms"] / tr), 3)
            except torch.cuda.OutOfMemoryError:
                rec["torch_fwd_bwd_ms"] = "out of memory"
            torch.cuda.empty_cache()
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
