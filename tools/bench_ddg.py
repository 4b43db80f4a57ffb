#!/usr/bin/env python3
"""What the episode recorder (BatchedRunner(record=True)) costs per step, and how long the probe and the teacher of the delta data
generation take.

    --mode step   bench_shield.py's protocol with record off or on: one warm-up run, then --repeats runs of --steps steps between HIP
                  events -> ms_per_step (median) and every run's figure; with record on, --steps more steps with the library's timing
                  hooks on, in a run of their own -> the recorder kernel's time per step (hook step_record) and the env step's next to it
                      cfg1   validation-random-seed-000, 1 instance x 32 agents, 2M     (64 steps x 5 runs)
                      cfg3   wfi_warehouse, 64 instances x 192 agents, 6M               (16 steps x 3 runs)
                  record off passes no argument, so the same file times a library built from the parent commit (tools/ab.py)
    --mode ddg    one recorded episode of the shape, then ddg.collect on it -> seconds of probe, pick and teacher, snapshots, picks
                      cfg1   1 instance x 32 agents        64x32   64 instances x 32 agents       (both validation-random-seed-000, 2M)

The weights are synthetic (seeded, untrained).  Prints ONE JSON line and appends it to profiles/bench_ddg.jsonl (or --out).

    python tools/bench_ddg.py --mode step --case cfg1 --record on
    python tools/bench_ddg.py --mode ddg --case 64x32 [--every 16]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mapf_gpt_amd import _lib, maps  # noqa: E402
from mapf_gpt_amd.model import build_model  # noqa: E402
from mapf_gpt_amd.runner import BatchedRunner, make_instances  # noqa: E402

# map, instances, agents, model, cap, steps, repeats
STEP_CASES = {"cfg1": ("validation-random-seed-000", 1, 32, "2M", 128, 64, 5), "cfg3": ("wfi_warehouse", 64, 192, "6M", 128, 16, 3)}
DDG_CASES = {"cfg1": ("validation-random-seed-000", 1, 32, "2M", 128), "64x32": ("validation-random-seed-000", 64, 32, "2M", 128)}


def bench_step(a):
    map_name, n_inst, n, model, cap, steps, repeats = STEP_CASES[a.case]
    steps, repeats = a.steps or steps, a.repeats or repeats
    grid, s_ok, g_ok = maps.load_named(map_name)
    net = build_model(model, seed=0, max_rows=min(n_inst * n, 16384), precision=a.precision)
    kw = {"record": True} if a.record == "on" else {}
    run = BatchedRunner(grid, n_inst, n, net, max_episode_steps=cap, seed=0, do_sample=True, precision=a.precision, **kw)
    pos, goal = make_instances(grid, n_inst, n, 0, s_ok, g_ok)
    ms = []
    for rep in range(repeats + 1):                                # run 0 warms up (lazy weight planes, the envelope probe)
        run.reset(pos, goal)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        run.run(steps)
        t1.record()
        t1.synchronize()
        if rep:
            ms.append(t0.elapsed_time(t1) / steps)
    per_step = {}
    if a.record == "on":
        run.reset(pos, goal)
        _lib.prof_reset()
        _lib.prof_enable(True)
        run.run(steps)
        hooks = _lib.prof_read()
        _lib.prof_enable(False)
        per_step = {k: round(hooks[k][0] / steps, 5) for k in ("step_record", "env_step") if k in hooks}
    return {"tool": "bench_ddg", "mode": "step", "case": a.case, "record": a.record, "weights": f"synthetic:{model}", "precision": a.precision,
            "instances": n_inst, "agents": n, "steps": steps, "ms_per_step": round(float(np.median(ms)), 4),
            "ms_per_step_runs": [round(float(x), 4) for x in ms], "kernel_ms_per_step": per_step,
            "record_bytes_per_step": n_inst * n * 5 if a.record == "on" else 0}


def bench_ddg(a):
    from mapf_gpt_amd import ddg
    map_name, n_inst, n, model, cap = DDG_CASES[a.case]
    grid, s_ok, g_ok = maps.load_named(map_name)
    net = build_model(model, seed=0, max_rows=min(n_inst * n, 16384), precision=a.precision)
    run = BatchedRunner(grid, n_inst, n, net, max_episode_steps=cap, seed=0, do_sample=True, precision=a.precision, record=True)
    pos, goal = make_instances(grid, n_inst, n, 0, s_ok, g_ok)
    keys = [{"map_name": map_name, "seed": i, "num_agents": n} for i in range(n_inst)]
    secs = []
    for rep in range(2):                                          # run 0 warms up
        run.reset(pos, goal)
        run.run(cap)
        out = ddg.collect(run, grid, goal, keys, every=a.every)
        secs.append(out["seconds"])
    picked = out["picked"]
    return {"tool": "bench_ddg", "mode": "ddg", "case": a.case, "weights": f"synthetic:{model}", "precision": a.precision, "instances": n_inst,
            "agents": n, "cap": cap, "every": a.every, "snapshots": out["probed"], "picked": int(picked.sum()),
            "teacher_solved": int(sum(r["metrics"]["CSR"] >= 1 for r in out["records"])), "rows": ddg.dataset_rows(out["records"]),
            "delta_mean": round(float(out["dmax"][picked].mean()), 2) if picked.any() else 0.0,
            "seconds": {k: round(float(v), 4) for k, v in secs[-1].items()}, "seconds_first": {k: round(float(v), 4) for k, v in secs[0].items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["step", "ddg"], required=True)
    ap.add_argument("--case", required=True)
    ap.add_argument("--record", choices=["off", "on"], default="off")
    ap.add_argument("--steps", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=0)
    ap.add_argument("--every", type=int, default=16)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_ddg.jsonl"))
    a = ap.parse_args()
    if a.case not in (STEP_CASES if a.mode == "step" else DDG_CASES):
        ap.error(f"--mode {a.mode} knows the cases {sorted(STEP_CASES if a.mode == 'step' else DDG_CASES)}")
    rec = bench_step(a) if a.mode == "step" else bench_ddg(a)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
