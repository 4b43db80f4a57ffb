#!/usr/bin/env python3
"""The reference tokenizer's rows along the seeded walks of tests/test_oracle_vs_reference.py (needs the reference build in
oracle/_ref: `make -C oracle ref` where the reference sources are available).  Writes tests/golden/refwalk_<walk>.npz with
    grid     uint8 [H, W]          the padded map
    pos      int32 [S, n, 2]       positions fed to update_agents at each step
    goal     int32 [S, n, 2]       goals fed at each step
    actions  int32 [S, n]          previous actions fed at each step (-1 at step 0)
    tokens   uint8 [S, n, 256]     what the reference's generate_observations returned
Run:  python tests/golden/make_golden_refwalk.py
"""
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import test_oracle_vs_reference as t  # noqa: E402

REF_DIR = os.path.join(ROOT, "oracle", "_ref")


def record(og, name, grid, steps):
    ref = og.ObservationGenerator(grid.astype(int).tolist(), og.InputParameters(20, 13, 5, 256, 5, 5, 64, False))
    tokens = []
    for k, (p, g, last) in enumerate(steps):
        pl, gl = [tuple(map(int, x)) for x in p], [tuple(map(int, x)) for x in g]
        if k == 0:
            ref.create_agents(pl, gl)
        ref.update_agents(pl, gl, [int(x) for x in last])
        tokens.append(np.array(ref.generate_observations(), dtype=np.uint8))
    out = os.path.join(t.GOLDEN, name + ".npz")
    np.savez_compressed(out, grid=grid.astype(np.uint8), pos=np.stack([s[0] for s in steps]).astype(np.int32),
                        goal=np.stack([s[1] for s in steps]).astype(np.int32),
                        actions=np.stack([s[2] for s in steps]).astype(np.int32), tokens=np.stack(tokens))
    print(out, os.path.getsize(out))


def main():
    if not glob.glob(os.path.join(REF_DIR, "observation_generator*.so")):
        sys.exit("oracle/_ref is not built: make -C oracle ref")
    sys.path.insert(0, REF_DIR)
    import observation_generator as og
    for case in t.RANDOM_CASES:
        record(og, t.random_name(*case), *t.random_walk(*case))
    for seed in t.CORNER_SEEDS:
        grid, steps, _ = t.corner_walk(seed)
        record(og, t.corner_name(seed), grid, steps)


if __name__ == "__main__":
    main()
