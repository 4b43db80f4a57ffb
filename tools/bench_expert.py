#!/usr/bin/env python3
"""Time and solve rates of the PIBT expert (mapf_gpt_amd/expert.py) and of the LaCAM search in front of it
(--algo lacam).

    --what time    three shapes: `dataset` 4096 instances x 32 agents on a 21 x 21 maze (the dataset's shape), `cfg3` 64 instances x 192
                   agents on wfi_warehouse (bench.py's cfg3 map), `one` 1 instance x 32 agents.  Per shape: one warm-up episode, then
                   --repeats episodes with HIP events around reset() (the BFS of every agent's distance field) and around run(steps)
                   (mgpt_expert_step: plan + env step + since update); then one more episode under the library's timing hooks for the
                   split of a step between the plan kernel and the env step.  ms per step = run time / steps; episodes per second =
                   instances / (reset + run).
    --what solve   solved episodes of six small shapes on seeded random maps (seed 7): the table of DESIGN section 20; then 256 instances
                   of 16, 24 and 32 agents on the dataset's 21 x 21 maze.
    --algo lacam   the same shapes with search="lacam" (--max-iters, --iters-per-launch).  solve adds the count of instances per search
                   status, the search's time per instance and its iterations; time adds the solve (HIP events around it, and the search
                   kernel's own time from the timing hooks), iterations per second and microseconds per iteration.

    --refine-rounds N   (--algo lacam) the refinement pass over found solutions, --refine-horizon H its horizon.
                   Records then carry the search's own status counts next to the final ones, the instances refined and rescued, the
                   sum of costs before and after and the rounds run; time adds the pass's kernels from the timing hooks and the solve
                   with the pass off on the same context.  A shape whose reach layers do not fit is reported as refused.

    --swap         the corridor swap rule in the generator, with either --algo; every record then carries
                   "swap": true, and time (pibt) adds the degree map's own time from the timing hooks.

    --lifelong     (--what time, pibt) lifelong episodes: every instance gets the queue evaluation.py seeds for run i,
                   reset() takes it, and a step is plan + env step + the tokenizer's update (goal check, the BFS of the agents whose
                   goal changed, next-action bits) + the post-step kernel; the split comes from the timing hooks over run(steps) alone.
                   Records carry "lifelong": true and throughput (arrivals per step and instance) in the place of solved counts.

Prints one JSON line per shape; --out FILE appends them there too.  Needs the GPU: there is no CPU path.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mapf_gpt_amd import _lib, maps  # noqa: E402
from mapf_gpt_amd.expert import BatchedExpert  # noqa: E402
from mapf_gpt_amd.runner import make_instances  # noqa: E402

TIME_SHAPES = {"dataset": ("maze21", 4096, 32, 128), "cfg3": ("wfi_warehouse", 64, 192, 128), "one": ("maze21", 1, 32, 128)}
# agents, (h, w, obstacle density), instances, step cap
SOLVE_SHAPES = [(4, (8, 8, 0.0), 32, 64), (8, (12, 12, 0.2), 32, 64), (32, (21, 21, 0.25), 32, 128), (64, (32, 32, 0.3), 16, 256),
                (70, (16, 16, 0.2), 16, 256), (3, (1, 12, 0.0), 16, 64)]
# the dataset's maze at three agent counts
MAZE_SHAPES = [(16, "maze21", 256, 128), (24, "maze21", 256, 128), (32, "maze21", 256, 128)]


SWAP = False                                         # --swap: every expert is built with the rule, every record says so


def emit(rec, out):
    if SWAP:
        rec = dict(rec, swap=True)
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def search_kw(a):
    if a.algo != "lacam":
        return {}
    return dict(search="lacam", max_iters=a.max_iters, iters_per_launch=a.iters_per_launch, refine_rounds=a.refine_rounds,
                refine_horizon=a.refine_horizon)


def refine_fields(ex, st, length):
    """What the refinement pass adds to a record (st, length: the final status and length)."""
    first, first_len, soc0, soc1, rounds, replans = (t.cpu().numpy() for t in ex.refine_stats())
    better, took = (length < first_len) | (soc1 < soc0), rounds > 0
    mean = lambda x, m: round(float(x[m].mean()), 2) if m.any() else None
    return {"refine_rounds": ex.refine_rounds, "first_status": {str(k): int((first == k).sum()) for k in (1, 2, 3, 4)},
            "refined": int(better.sum()), "rescued": int(((first == 4) & (st == 1)).sum()), "replans": int(replans.sum()),
            "max_rounds_of_an_instance": int(rounds.max()), "mean_first_length_of_refined": mean(first_len, took),
            "mean_length_of_refined": mean(length, took), "mean_soc_before_of_refined": mean(soc0, took),
            "mean_soc_after_of_refined": mean(soc1, took), "mean_first_length_of_first_status_1": mean(first_len, first == 1),
            "mean_soc_before_of_first_status_1": mean(soc0, first == 1), "mean_soc_after_of_status_1": mean(soc1, st == 1)}


def search_fields(ex, search_ms, kernel_ms=None):
    """What a solve adds to a record: status counts, iterations, the search's time per instance and per iteration."""
    st, it, nodes, length = (t.cpu().numpy() for t in ex.search_stats())
    total = int(it.sum())
    rec = {"max_iters": ex.max_iters, "status": {str(k): int((st == k).sum()) for k in (1, 2, 3, 4)}, "iterations": total,
           "max_iterations_of_an_instance": int(it.max()), "nodes": int(nodes.sum()), "search_ms": round(search_ms, 3),
           "search_ms_per_instance": round(search_ms / len(st), 4), "iterations_per_s": round(total / max(search_ms * 1e-3, 1e-9), 1),
           "us_per_iteration_of_the_longest_instance": round(search_ms * 1e3 / max(int(it.max()), 1), 3),
           "mean_length_of_status_1": round(float(length[st == 1].mean()), 2) if (st == 1).any() else None}
    if kernel_ms is not None:
        rec["search_kernel_ms"] = round(kernel_ms[0], 3)
        rec["search_launches"] = int(kernel_ms[1])
    if ex.refine_rounds:
        rec.update(refine_fields(ex, st, length))
    return rec


def time_search(name, a):
    """The solve of one timing shape: reset() = BFS + search, the search alone from the stream's events around mgpt_expert_solve."""
    map_name, n_inst, n, steps = TIME_SHAPES[name]
    if map_name == "maze21":
        grid, s_ok, g_ok = maps.pad(maps.maze_map(21, 21, 7)), None, None
    else:
        grid, s_ok, g_ok = maps.load_named(map_name)
    pos, goal = make_instances(grid, n_inst, n, 0, s_ok, g_ok)
    try:
        ex = BatchedExpert(grid, n_inst, n, steps, seed=7, swap=SWAP, **search_kw(a))
    except _lib.MGPTError as e:
        if e.code != _lib.ERR_UNSUPPORTED:
            raise
        emit({"tool": "bench_expert", "what": "time", "algo": "lacam", "shape": name, "map": map_name, "instances": n_inst, "agents": n,
              "refused": str(e)}, a.out)
        return
    h = ex._h

    def solves():
        out = []
        for rep in range(a.repeats + 1):             # episode 0 warms up
            ex.search = None                         # reset without the solve, then the solve alone between two events
            ex.reset(pos, goal)
            ex.search = "lacam"
            with _lib.on_device(ex.device):
                ms = timed(lambda: _lib.check(_lib.lib().mgpt_expert_solve(h, _lib.stream_ptr())))
            if rep:
                out.append(ms)
        return out

    off_ms = None
    if a.refine_rounds:                              # the same context with the pass off, then on again
        ex.set_refine(0)
        off_ms = solves()
        ex.run(steps)                                # the switch is refused in the middle of an episode: run this one to its end
        ex.set_refine(a.refine_rounds, a.refine_horizon)
    solve_ms = solves()
    _lib.prof_enable(True)
    _lib.prof_reset()
    ex.reset(pos, goal)
    prof = _lib.prof_read()
    _lib.prof_enable(False)
    run_ms = timed(lambda: ex.run(steps))
    m = ex.metrics().cpu().numpy()
    rec = {"tool": "bench_expert", "what": "time", "algo": "lacam", "shape": name, "map": map_name, "instances": n_inst, "agents": n,
           "steps": steps, "iters_per_launch": a.iters_per_launch, "solve_ms_runs": [round(x, 3) for x in solve_ms]}
    rec.update(search_fields(ex, float(np.median(solve_ms)), prof.get("expert_lacam_search", (0.0, 0))))
    if a.refine_rounds:
        rec["solve_ms_runs_with_the_pass_off"] = [round(x, 3) for x in off_ms]
        for k in ("path", "round", "final"):
            ms, launches = prof.get("expert_refine_" + k, (0.0, 0))
            rec["refine_%s_ms" % k], rec["refine_%s_launches" % k] = round(ms, 3), int(launches)
    rec.update({"ms_run_after_solve": round(run_ms, 3), "solved": int(m[:, 0].sum()), "mean_isr": round(float(m[:, 1].mean()), 4)})
    emit(rec, a.out)


def lifelong_queues(grid, g_ok, n_inst, n):
    from mapf_gpt_amd import evaluation as ev
    frame = (grid, None, np.ones(grid.shape, bool) if g_ok is None else g_ok)
    cells = ev.lifelong_cells(frame)
    return torch.from_numpy(np.stack([ev.lifelong_queue(frame, i, n, cells=cells) for i in range(n_inst)]))


def time_lifelong(name, repeats, out):
    map_name, n_inst, n, steps = TIME_SHAPES[name]
    if map_name == "maze21":
        grid, s_ok, g_ok = maps.pad(maps.maze_map(21, 21, 7)), None, None
    else:
        grid, s_ok, g_ok = maps.load_named(map_name)
    pos, goal = make_instances(grid, n_inst, n, 0, s_ok, g_ok)
    queue = lifelong_queues(grid, g_ok, n_inst, n)
    ex = BatchedExpert(grid, n_inst, n, steps, seed=7, swap=SWAP, lifelong=True)
    reset_ms, run_ms = [], []
    for rep in range(repeats + 1):                   # episode 0 warms up (code objects, allocations)
        r = timed(lambda: ex.reset(pos, goal, queue))
        s = timed(lambda: ex.run(steps))
        if rep:
            reset_ms.append(r)
            run_ms.append(s)
    arrivals = ex.arrivals().sum(1).cpu().numpy()
    dirty = float(ex.env.goals_reached().sum().item()) / (steps * n_inst * n)
    ex.reset(pos, goal, queue)                       # the split, over the steps of an episode of its own (the hooks add events to every launch)
    _lib.prof_enable(True)
    _lib.prof_reset()
    ex.run(steps)
    prof = _lib.prof_read()
    _lib.prof_enable(False)
    names = {"plan": ("expert_pibt_plan",), "env": ("env_step",), "tok_update": ("tok_update_agents",), "tok_bfs": ("bfs_distance_field",),
             "tok_next": ("tok_next_action",), "post": ("expert_lifelong_post",)}
    k = {key: round(sum(prof.get(x, (0.0, 0))[0] for x in xs) / steps, 4) for key, xs in names.items()}
    total = max(sum(k.values()), 1e-9)
    r, s = float(np.median(reset_ms)), float(np.median(run_ms))
    emit({"tool": "bench_expert", "what": "time", "lifelong": True, "shape": name, "map": map_name, "instances": n_inst, "agents": n,
          "steps": steps, "queue": int(queue.shape[2]), "ms_per_step": round(s / steps, 4), "ms_run": round(s, 3),
          "ms_runs": [round(x, 3) for x in run_ms], "ms_reset": round(r, 3), "episodes_per_s": round(n_inst / ((r + s) * 1e-3), 1),
          "kernel_ms_per_step": k, "tokenizer_update_ms_per_step": round(k["tok_update"] + k["tok_bfs"] + k["tok_next"], 4),
          "field_rebuild_share_of_kernel_time": round(k["tok_bfs"] / total, 3),
          "tokenizer_update_share_of_kernel_time": round((k["tok_update"] + k["tok_bfs"] + k["tok_next"]) / total, 3),
          "dirty_agents_per_step_share": round(dirty, 5), "arrivals_per_step_per_instance": round(float(arrivals.mean()) / steps, 4),
          "min_arrivals_of_an_instance": int(arrivals.min())}, out)


def time_shape(name, repeats, out):
    map_name, n_inst, n, steps = TIME_SHAPES[name]
    if map_name == "maze21":
        grid, s_ok, g_ok = maps.pad(maps.maze_map(21, 21, 7)), None, None
    else:
        grid, s_ok, g_ok = maps.load_named(map_name)
    pos, goal = make_instances(grid, n_inst, n, 0, s_ok, g_ok)
    if SWAP:                                         # the degree map is built by the constructor, once
        _lib.prof_enable(True)
        _lib.prof_reset()
    ex = BatchedExpert(grid, n_inst, n, steps, seed=7, swap=SWAP)
    extra = {}
    if SWAP:
        extra["cell_degree_ms"] = round(_lib.prof_read().get("expert_cell_degree", (0.0, 0))[0], 4)
        _lib.prof_enable(False)
    reset_ms, run_ms = [], []
    for rep in range(repeats + 1):                   # episode 0 warms up (code objects, allocations)
        r = timed(lambda: ex.reset(pos, goal))
        s = timed(lambda: ex.run(steps))
        if rep:
            reset_ms.append(r)
            run_ms.append(s)
    m = ex.metrics().cpu().numpy()
    _lib.prof_enable(True)                           # the split, in an episode of its own: the hooks add events to every launch
    _lib.prof_reset()
    ex.reset(pos, goal)
    ex.run(steps)
    prof = _lib.prof_read()
    _lib.prof_enable(False)
    plan, env, bfs = (prof.get(k, (0.0, 0))[0] for k in ("expert_pibt_plan", "env_step", "bfs_distance_field"))
    r, s = float(np.median(reset_ms)), float(np.median(run_ms))
    emit({"tool": "bench_expert", "what": "time", "shape": name, "map": map_name, "instances": n_inst, "agents": n, "steps": steps,
          "ms_per_step": round(s / steps, 4), "ms_run": round(s, 3), "ms_runs": [round(x, 3) for x in run_ms], "ms_reset": round(r, 3),
          "episodes_per_s": round(n_inst / ((r + s) * 1e-3), 1), "plan_ms_per_step": round(plan / steps, 4),
          "env_ms_per_step": round(env / steps, 4), "plan_share_of_plan_plus_env": round(plan / max(plan + env, 1e-9), 3),
          "kernel_ms_per_step": {"plan": round(plan / steps, 4), "env": round(env / steps, 4)},      # (the keys tools/ab.py records)
          "bfs_ms_of_reset": round(bfs, 3), "solved": int(m[:, 0].sum()), "mean_isr": round(float(m[:, 1].mean()), 4), **extra}, out)


def solve_shape(n, hwd, n_inst, cap, a):
    if hwd == "maze21":
        grids, label = maps.pad(maps.maze_map(21, 21, 7)), "21x21 maze"
        pos, goal = make_instances(grids, n_inst, n, 0, None, None)
    else:
        h, w, density = hwd
        label = f"{h}x{w} at {density:.0%}"
        grids = np.stack([maps.pad(maps.random_map(h, w, density, 7000 + i)) for i in range(n_inst)])
        pos = np.empty((n_inst, n, 2), np.int16)
        goal = np.empty((n_inst, n, 2), np.int16)
        for i in range(n_inst):
            pos[i], goal[i] = maps.place_agents(grids[i], n, 7 + i)
        pos, goal = torch.from_numpy(pos), torch.from_numpy(goal)
    ex = BatchedExpert(grids, n_inst, n, cap, seed=7, swap=SWAP, **search_kw(a))
    reset_ms = timed(lambda: ex.reset(pos, goal))
    ex.run(cap)
    m = ex.metrics().cpu().numpy()
    ok = m[:, 0] >= 1
    rec = {"tool": "bench_expert", "what": "solve", "algo": a.algo, "agents": n, "map": label, "instances": n_inst, "step_cap": cap,
           "solved": int(ok.sum()), "mean_length_of_solved": round(float(m[ok, 4].mean()), 2) if ok.any() else None,
           "mean_isr": round(float(m[:, 1].mean()), 4)}
    if a.algo == "lacam":                             # reset = BFS + search; the first shape's figure includes the code object's load
        rec.update(search_fields(ex, reset_ms))
        replayed = ex.search_stats()[0].cpu().numpy() == 1
        rec["mean_soc_of_status_1"] = round(float(m[replayed, 2].mean()), 2) if replayed.any() else None
        rec["search_ms_includes"] = "reset (BFS)"
    emit(rec, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["time", "solve"], required=True)
    ap.add_argument("--shapes", nargs="*", default=None, help="time: a subset of " + " ".join(TIME_SHAPES))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    ap.add_argument("--algo", choices=["pibt", "lacam"], default="pibt")
    ap.add_argument("--max-iters", type=int, default=4096)
    ap.add_argument("--iters-per-launch", type=int, default=None, help="default: the library's slice")
    ap.add_argument("--swap", action="store_true", help="the corridor swap rule in the generator")
    ap.add_argument("--refine-rounds", type=int, default=0, help="--algo lacam: rounds of the refinement pass (0 = off)")
    ap.add_argument("--refine-horizon", type=int, default=None, help="default: twice the step cap")
    ap.add_argument("--maze-only", action="store_true", help="solve: the three maze shapes only")
    ap.add_argument("--lifelong", action="store_true", help="time (pibt): lifelong episodes on evaluation.py's seeded queues")
    a = ap.parse_args()
    global SWAP
    SWAP = a.swap
    _lib.require_gpu()
    if a.lifelong and (a.what != "time" or a.algo != "pibt"):
        ap.error("--lifelong goes with --what time and --algo pibt")
    if a.what == "time":
        for name in a.shapes or list(TIME_SHAPES):
            if a.lifelong:
                time_lifelong(name, a.repeats, a.out)
            elif a.algo == "lacam":
                time_search(name, a)
            else:
                time_shape(name, a.repeats, a.out)
    else:
        if a.refine_rounds and a.algo != "lacam":
            ap.error("--refine-rounds needs --algo lacam")
        for n, hwd, n_inst, cap in ([] if a.maze_only else SOLVE_SHAPES) + MAZE_SHAPES:
            solve_shape(n, hwd, n_inst, cap, a)


if __name__ == "__main__":
    main()
