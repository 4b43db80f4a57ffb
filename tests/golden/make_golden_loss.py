#!/usr/bin/env python3
"""Goldens of GPT.forward(idx, targets) from the REAL reference (build container only), in the style of make_golden.py.

For the tiny and 6M shapes on seeded synthetic weights: 4 token rows, targets mixing the patterns the reference meets
(row 0: every position targeted; row 1: position 255 only, the dataset's pattern, fast_data_loader.py:34,58; row 2: all -1;
row 3: about half of the positions), and what mapf_gpt/model.py:167-189 returns for them: the loss and the logits at 16 fixed
positions.  Tests only read the .npz files.
Run:  python tests/golden/make_golden_loss.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
OUT = os.path.join(ROOT, "tests", "golden")

from mapf_gpt_amd import weights  # noqa: E402
from make_golden import import_reference  # noqa: E402

POSITIONS = np.array([0, 1, 2, 17, 31, 32, 63, 64, 100, 127, 128, 191, 200, 253, 254, 255], np.int64)


def cases(seed=5):
    rng = np.random.Generator(np.random.PCG64(seed))
    tokens = rng.integers(0, 67, (4, 256)).astype(np.uint8)
    targets = np.full((4, 256), -1, np.int64)
    targets[0] = rng.integers(0, 67, 256)
    targets[1, 255] = rng.integers(0, 5)
    half = rng.random(256) < 0.5
    targets[3, half] = rng.integers(0, 67, int(half.sum()))
    return tokens, targets


def main():
    import torch
    _, GPT, GPTConfig = import_reference()
    torch.manual_seed(0)
    tokens, targets = cases()
    for name in ("tiny", "6M"):
        args = weights.model_args(name)
        sd = weights.synthetic_state_dict(name, seed=3, scale=1.0)
        net = GPT(GPTConfig(**args)).eval()
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        with torch.no_grad():
            logits, loss = net(torch.from_numpy(tokens.astype(np.int64)), torch.from_numpy(targets))     # model.py:180-184
        out = dict(tokens=tokens, targets=targets, loss=np.array(float(loss), np.float64), positions=POSITIONS,
                   logits=logits[:, POSITIONS, :].numpy().astype(np.float32), seed=np.array(3), scale=np.array(1.0))
        np.savez_compressed(os.path.join(OUT, f"loss_{name}.npz"), **out)
        print(name, "loss", float(loss), "logits", out["logits"].shape)


if __name__ == "__main__":
    main()
