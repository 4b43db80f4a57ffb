#!/usr/bin/env python3
"""What BatchedRunner(retire_done=True) saves, and what it costs where nothing retires.

    case A   6M f16x3, puzzle-00, 4096 instances x 1 agent, 64 steps: episodes finish all along the run; the time should follow
             rows_forwarded / (rows x steps)
    case B   bench.py's cfg3 shape (wfi_warehouse, 64 instances x 192 agents, 6M), 16 steps: nothing finishes, so the difference
             between the modes is the mode's overhead -- one gather of the token rows per step and one 4-byte read-back per poll

One batch, one warm-up episode, then --repeats episodes timed with HIP events around run().  Prints ONE JSON line.  --mode plain
passes no retire argument to the runner, so the same file times a checkout that predates the mode.

    python tools/bench_retire.py --case A --mode retire [--poll-every 8] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mapf_gpt_amd import maps  # noqa: E402
from mapf_gpt_amd.model import build_model  # noqa: E402
from mapf_gpt_amd.runner import BatchedRunner, make_instances  # noqa: E402

CASES = {"A": ("puzzle-00", 4096, 1, 64), "B": ("wfi_warehouse", 64, 192, 16)}      # map, instances, agents, steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES), required=True)
    ap.add_argument("--mode", choices=["plain", "retire"], required=True)
    ap.add_argument("--poll-every", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--out", default=None, help="append the JSON line to this file too")
    a = ap.parse_args()
    map_name, n_inst, n, steps = CASES[a.case]
    grid, s_ok, g_ok = maps.load_named(map_name)
    rows = n_inst * n
    net = build_model("6M", seed=0, max_rows=min(rows, 16384), precision=a.precision)
    pos, goal = make_instances(grid, n_inst, n, 0, s_ok, g_ok)
    kw = {"retire_done": True, "poll_every": a.poll_every} if a.mode == "retire" else {}
    run = BatchedRunner(grid, n_inst, n, net, max_episode_steps=128, seed=0, do_sample=True, precision=a.precision, **kw)
    ms = []
    for rep in range(a.repeats + 1):                 # episode 0 warms up (lazy weight planes, the envelope probe)
        run.reset(pos, goal)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        run.run(steps)
        t1.record()
        t1.synchronize()
        if rep:
            ms.append(t0.elapsed_time(t1))
    done = run.env.sync_state()[2].cpu().numpy()
    rec = {"tool": "bench_retire", "case": a.case, "mode": a.mode, "precision": a.precision, "instances": n_inst, "agents": n, "steps": steps,
           "poll_every": a.poll_every if a.mode == "retire" else None, "ms_per_run": round(float(np.median(ms)), 3),
           "ms_runs": [round(float(x), 3) for x in ms], "steps_run": run.t,
           "rows_forwarded": int(getattr(run, "rows_forwarded", rows * run.t)), "rows_x_steps": rows * steps,
           "instances_done_at_end": int(np.count_nonzero(done))}
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
