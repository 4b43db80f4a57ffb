#!/usr/bin/env python3
"""Cost of the evaluation entry points against the default forward (f16x3 by default):

    mgpt_gpt_forward                      last-position logits (the act path's forward)
    mgpt_gpt_forward_seq, targets only    every position's last layer + ln_f + head + cross-entropy, no logits written
    mgpt_gpt_forward_seq, with logits     ... and the [rows][256][67] logits
    mgpt_gpt_score_last                   the forward of mgpt_gpt_forward + per-row NLL and hit

on the 6M shape with 12 288 rows and the 2M shape with 16 384 rows (one call of all rows each, max_rows = rows), median of --reps
HIP-event-timed calls after --warmup, then the per-class profiler split of one call of each.

    python tools/bench_loss.py [--precision f16x3] [--reps 10] [--warmup 3] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mapf_gpt_amd import _lib  # noqa: E402
from mapf_gpt_amd.model import build_model  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.lib()
    prec = _lib.PRECISIONS[a.precision]
    lines = []
    for shape, rows in (("6M", 12288), ("2M", 16384)):
        net = build_model(shape, seed=0, max_rows=rows, precision=a.precision)
        rng = np.random.Generator(np.random.PCG64(0))
        tok = torch.from_numpy(rng.integers(0, 67, (rows, 256)).astype(np.uint8)).cuda()
        tg = torch.full((rows, 256), -1, dtype=torch.int32, device="cuda")
        tg[:, -1] = torch.from_numpy(rng.integers(0, 5, rows).astype(np.int32)).cuda()
        lg = torch.empty((rows, 67), device="cuda")
        lg_all = torch.empty((rows, 256, 67), device="cuda")
        nll = torch.empty(rows, device="cuda")
        cnt = torch.empty(rows, dtype=torch.int32, device="cuda")
        hit = torch.empty(rows, dtype=torch.int32, device="cuda")
        h, P, sp = net._h, _lib.ptr, _lib.stream_ptr
        calls = {
            "forward": lambda: _lib.check(L.mgpt_gpt_forward(h, P(tok), rows, P(lg), prec, sp())),
            "forward_seq_targets": lambda: _lib.check(L.mgpt_gpt_forward_seq(h, P(tok), rows, 256, None, P(tg), P(nll), P(cnt), prec, sp())),
            "forward_seq_logits": lambda: _lib.check(L.mgpt_gpt_forward_seq(h, P(tok), rows, 256, P(lg_all), P(tg), P(nll), P(cnt), prec, sp())),
            "score_last": lambda: _lib.check(L.mgpt_gpt_score_last(h, P(tok), rows, P(tg[:, -1].contiguous()), P(nll), P(hit), None, prec, sp())),
        }
        res = {}
        for k, fn in calls.items():
            res[k] = timed(fn, a.reps, a.warmup)
        base = res["forward"][0]
        for k, (med, mn) in res.items():
            lines.append(f"{shape} rows={rows} {a.precision} {k:22s} median {med:8.3f} ms  min {mn:8.3f} ms  x forward {med / base:.3f}")
        for k, fn in calls.items():
            _lib.prof_reset()
            _lib.prof_enable(True)
            fn()
            split = _lib.prof_read()
            _lib.prof_enable(False)
            lines.append(f"{shape} {k} profiler split: " + json.dumps({n: round(v[0], 3) for n, v in sorted(split.items()) if v[1]}))
        del net
        torch.cuda.empty_cache()
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
