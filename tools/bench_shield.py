#!/usr/bin/env python3
"""What the collision shield (BatchedRunner(shield="pibt")) costs per step and what it does to the episodes.

    cfg1   bench.py's cfg1 shape: validation-random-seed-000, 1 instance x 32 agents, 2M
    cfg3   bench.py's cfg3 shape: wfi_warehouse, 64 instances x 192 agents, 6M

Two measurements per run, shield off or on:
    time      one warm-up episode, then --repeats runs of --steps steps between HIP events -> ms_per_step (median) and every run's figure;
              then --steps more steps with the library's timing hooks on -> the shield kernel's own time per step (hook expert_shield)
              and the env step's next to it
    episodes  --episodes whole episodes (instances seeded apart: episode e uses seeds e * instances ..) -> mean CSR, ISR, SoC, makespan
              and, with the shield on, the override rate (overrides / (ep_length x agents))

--lifelong runs the same two measurements on lifelong episodes (on_target = restart): every instance gets the seeded
goal queue of evaluation.lifelong_queue (seed = the instance's), shield on is BatchedRunner(shield="pibt", shield_lifelong=True), the
post-step kernel's time is reported next to the shield's (hook expert_shield_lifelong_post) and the episodes' figure is the throughput
(arrivals per step and instance) in the place of CSR .. makespan.

The weights are synthetic (seeded, untrained): the metrics say what the shield does to a policy that knows nothing, not to a trained one.
Prints ONE JSON line and appends it to profiles/bench_shield.jsonl (or --out).

    python tools/bench_shield.py --case cfg1 --shield on [--lifelong] [--steps 64] [--repeats 5] [--episodes 2] [--precision f16x3]
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

CASES = {"cfg1": ("validation-random-seed-000", 1, 32, "2M", 128), "cfg3": ("wfi_warehouse", 64, 192, "6M", 128)}   # map, instances, agents, model, cap


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES), required=True)
    ap.add_argument("--shield", choices=["off", "on"], required=True)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--episodes", type=int, default=2)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--lifelong", action="store_true", help="lifelong episodes on evaluation.lifelong_queue's queues (DESIGN.md section 35)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_shield.jsonl"))
    a = ap.parse_args()
    map_name, n_inst, n, model, cap = CASES[a.case]
    grid, s_ok, g_ok = maps.load_named(map_name)
    net = build_model(model, seed=0, max_rows=min(n_inst * n, 16384), precision=a.precision)
    kw = {"shield": "pibt"} if a.shield == "on" else {}          # (off passes nothing: the same file times a checkout without the argument)
    if a.lifelong and a.shield == "on":
        kw["shield_lifelong"] = True
    run = BatchedRunner(grid, n_inst, n, net, max_episode_steps=cap, seed=0, do_sample=True, precision=a.precision, **kw)
    pos, goal = make_instances(grid, n_inst, n, 0, s_ok, g_ok)

    def queues(first_seed):
        """--lifelong: {"goal_queue": int16 [n_inst, n, LIFELONG_QUEUE, 2]}, instance i seeded first_seed + i; else no argument."""
        if not a.lifelong:
            return {}
        from mapf_gpt_amd import evaluation as ev
        frame = (grid, s_ok, g_ok)
        cells = ev.lifelong_cells(frame)
        return {"goal_queue": torch.from_numpy(np.stack([ev.lifelong_queue(frame, first_seed + i, n, cells=cells) for i in range(n_inst)]))}

    ms = []
    for rep in range(a.repeats + 1):                              # run 0 warms up (lazy weight planes, the envelope probe)
        run.reset(pos, goal, **queues(0))
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        run.run(a.steps)
        t1.record()
        t1.synchronize()
        if rep:
            ms.append(t0.elapsed_time(t1) / a.steps)
    run.reset(pos, goal, **queues(0))
    _lib.prof_reset()
    _lib.prof_enable(True)
    run.run(a.steps)
    hooks = _lib.prof_read()
    _lib.prof_enable(False)
    per_step = {k: round(hooks[k][0] / a.steps, 4) for k in ("expert_shield", "expert_shield_lifelong_post", "env_step") if k in hooks}

    metrics, rates, arrivals = [], [], []
    for e in range(a.episodes):
        p, g = make_instances(grid, n_inst, n, e * n_inst, s_ok, g_ok)
        run.reset(p, g, **queues(e * n_inst))
        run.run(cap)
        m = run.metrics().cpu().numpy()
        metrics.append(m)
        if a.lifelong:
            arrivals.append(run.env.goals_reached().sum(1).cpu().numpy())
        if a.shield == "on":
            rates.append(run.shield_overrides().cpu().numpy() / np.maximum(1.0, m[:, 4] * n))
    m = np.concatenate(metrics)
    rec = {"tool": "bench_shield", "case": a.case, "shield": a.shield, "weights": f"synthetic:{model}", "precision": a.precision,
           "instances": n_inst, "agents": n, "steps": a.steps, "ms_per_step": round(float(np.median(ms)), 4),
           "ms_per_step_runs": [round(float(x), 4) for x in ms], "kernel_ms_per_step": per_step, "episodes": int(len(m)),
           "CSR": round(float(m[:, 0].mean()), 4), "ISR": round(float(m[:, 1].mean()), 4), "SoC": round(float(m[:, 2].mean()), 2),
           "makespan": round(float(m[:, 3].mean()), 2),
           "override_rate": round(float(np.concatenate(rates).mean()), 4) if rates else None}
    if a.lifelong:                                               # no CSR .. makespan in a lifelong episode: arrivals per step and instance
        for k in ("CSR", "ISR", "SoC", "makespan"):
            del rec[k]
        rec.update(lifelong=True, throughput=round(float(np.concatenate(arrivals).mean()) / cap, 4),
                   arrivals_min=int(np.concatenate(arrivals).min()), arrivals_max=int(np.concatenate(arrivals).max()))
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
