#!/usr/bin/env python3
"""Expert episodes to training rows: the batched route (BatchedExpert.dataset_rows) against the per-episode route
it stands next to (records() -> ObservationGenerator.generate_observations_device), on the same episodes in the same process.

    --mode rows   one 21 x 21 maze (frame 31 x 31), 128-step cap, BatchedExpert(swap=True): 100 seeds at 16, 24 and 32 agents = 300
                  episodes in three contexts.  Each route turns all three contexts' episodes into (rows, labels) on the device; a route's
                  time is a host clock from its first call to a device synchronise after its last.  One warm-up of each route (tables,
                  lazy allocations), then --repeats pairs, batched first in odd pairs and the loop first in even ones -> median and range
                  per route.  Then one more batched pass with the library's timing hooks on -> kernel ms under ds_paths and
                  ds_episode_tokens and their share of that pass's host time, and one hooked pass of the loop -> kernel ms under
                  tok_generate_observations (ds_tokens_kernel) and tok_update_agents (ds_records_kernel).  For tools/ab.py the line also
                  carries ms_per_step (the batched median) and kernel_ms_per_step (all those hooks).  The two routes' rows are compared
                  before anything is timed.
    --mode e2e    a 4-map config (two 21 x 21 mazes, two 21 x 21 random maps at 15 %), --seeds seeds x 16 / 24 / 32 agents, 128-step cap,
                  PIBT with the swap rule, from a YAML written to a temporary folder:
                      log     python -m mapf_gpt_amd.expert --out  +  split_by_map  +  build_shards (dataset_build --logs)
                      shards  python -m mapf_gpt_amd.expert --shards
                  each once after a warm-up run of the shards route, as functions of this process; the two sets of .arrow files are
                  compared byte for byte.

    --mode rows --lifelong   the same schedule on BatchedExpert(lifelong=True, swap=True) with the evaluation's seeded goal queues (DESIGN.md
                  section 34): BatchedExpert.lifelong_rows against records() -> generate_observations_device; every episode runs the
                  whole cap and is kept.  Kernel ms under ds_paths_lifelong and ds_episode_tokens_lifelong.

Prints ONE JSON line and appends it to profiles/bench_episode_rows.jsonl (bench_episode_rows_lifelong.jsonl with --lifelong; or --out).
"""
import argparse
import contextlib
import glob
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mapf_gpt_amd import _lib, maps  # noqa: E402

AGENTS, CAP, SIDE = (16, 24, 32), 128, 21


def map_string(obst):
    return "\n".join("".join("#" if v else "." for v in row) for row in obst)


def clock():
    torch.cuda.synchronize()
    return time.perf_counter()


def bench_rows(a):
    from mapf_gpt_amd.dataset_tokenizer import ObservationGenerator, TableCache
    from mapf_gpt_amd.expert import BatchedExpert
    obst = maps.maze_map(SIDE, SIDE, 7)
    grid = maps.pad(obst)
    named = {"maze21": map_string(obst)}
    runs = []
    frame = (grid, grid == 0, grid == 0)
    for n in AGENTS:
        pos = np.empty((a.seeds, n, 2), np.int16)
        goal = np.empty_like(pos)
        for s in range(a.seeds):
            pos[s], goal[s] = maps.place_agents(grid, n, s)
            while a.lifelong and (pos[s] == goal[s]).all(-1).any():      # an agent that starts on its goal advances its list with no arrival:
                goal[s] = np.roll(goal[s], 1, axis=0)                   # both routes raise the reference's IndexError on such a log
        ex = BatchedExpert(grid, a.seeds, n, CAP, seed=0, swap=True, lifelong=a.lifelong)
        if a.lifelong:
            from mapf_gpt_amd import evaluation as ev
            cells = ev.lifelong_cells(frame)
            queue = np.stack([ev.lifelong_queue(frame, s, n, cells=cells) for s in range(a.seeds)])
            ex.reset(torch.from_numpy(pos), torch.from_numpy(goal), torch.from_numpy(queue))
        else:
            ex.reset(torch.from_numpy(pos), torch.from_numpy(goal))
        ex.run(CAP)
        runs.append((ex, pos, [{"map_name": "maze21", "seed": s, "num_agents": n} for s in range(a.seeds)]))
    cache = TableCache()

    def batched():
        if a.lifelong:
            return [ex.lifelong_rows(pos, tables=cache)[0][1:] for ex, pos, _ in runs]
        return [ex.dataset_rows(pos, tables=cache)[0][1:] for ex, pos, _ in runs]

    def loop():
        out = []
        for ex, pos, keys in runs:
            recs = ex.records(keys, pos)
            out.append(ObservationGenerator(named, recs).generate_observations_device(0, len(recs)))
        return out

    def timed(f):
        t0 = clock()
        f()
        return clock() - t0

    got, want = batched(), loop()                                  # warm-up of both, and the check
    same = all(torch.equal(x, wx) and torch.equal(y, wy) for (x, y), (wx, wy) in zip(got, want))
    rows = sum(int(x.shape[0]) for x, _ in got)
    solved = sum(int((ex.metrics()[:, 0] >= 1).sum()) for ex, _, _ in runs)
    arrivals = sum(int(ex.env.goals_reached().sum()) for ex, _, _ in runs) if a.lifelong else None
    del got, want
    tb, tl = [], []
    for rep in range(a.repeats):
        for name in (("batched", "loop") if rep % 2 == 0 else ("loop", "batched")):
            (tb if name == "batched" else tl).append(timed(batched if name == "batched" else loop))
    _lib.prof_reset()
    _lib.prof_enable(True)
    t_hook = timed(batched)
    hooks = _lib.prof_read()
    kern = {k: round(hooks[k][0], 4) for k in ("ds_paths", "ds_episode_tokens", "ds_paths_lifelong", "ds_episode_tokens_lifelong") if k in hooks}
    _lib.prof_reset()
    timed(loop)                                                    # one hooked pass of the per-episode route: ds_records / ds_tokens
    hooks = _lib.prof_read()
    _lib.prof_enable(False)
    per_episode = {k: round(hooks[k][0], 4) for k in ("tok_generate_observations", "tok_update_agents") if k in hooks}

    def stats(t):
        return {"median_s": round(float(np.median(t)), 5), "min_s": round(min(t), 5), "max_s": round(max(t), 5),
                "us_per_row": round(1e6 * float(np.median(t)) / max(rows, 1), 4)}

    kind = {"mode": "rows", "lifelong": True, "arrivals": arrivals} if a.lifelong else {"mode": "rows", "solved": solved}
    return {"tool": "bench_episode_rows", **kind, "map": f"maze {SIDE}x{SIDE}", "episodes": a.seeds * len(AGENTS),
            "rows": rows, "rows_equal": bool(same), "repeats": a.repeats, "batched": stats(tb), "loop": stats(tl),
            "speedup": round(float(np.median(tl)) / float(np.median(tb)), 2), "kernel_ms": kern,
            "kernel_share_of_pass": round(sum(kern.values()) / (1e3 * t_hook), 4), "hooked_pass_s": round(t_hook, 5),
            # the two keys tools/ab.py records: a "step" is one batched pass
            "ms_per_step": round(1e3 * float(np.median(tb)), 3), "kernel_ms_per_step": {**kern, **per_episode}}


def bench_e2e(a):
    import yaml
    from mapf_gpt_amd import dataset_build as db
    from mapf_gpt_amd import expert
    named = {"bench-mazes-0": map_string(maps.maze_map(SIDE, SIDE, 7)), "bench-mazes-1": map_string(maps.maze_map(SIDE, SIDE, 8)),
             "bench-random-0": map_string(maps.random_map(SIDE, SIDE, 0.15, 9)), "bench-random-1": map_string(maps.random_map(SIDE, SIDE, 0.15, 10))}
    cfg = {"environment": {"name": "Environment", "with_animation": False, "on_target": "nothing", "max_episode_steps": CAP,
                           "observation_type": "MAPF", "collision_system": "soft", "seed": {"grid_search": list(range(a.seeds))},
                           "num_agents": {"grid_search": list(AGENTS)}, "map_name": {"grid_search": list(named)}}}
    desired = 10 ** 9                                              # everything: both routes write every kept row
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "cfg.yaml"), "w") as f:
            yaml.safe_dump(cfg, f, sort_keys=False)
        with open(os.path.join(d, "maps.yaml"), "w") as f:
            yaml.safe_dump(named, f)
        base = ["--config", os.path.join(d, "cfg.yaml"), "--maps", os.path.join(d, "maps.yaml"), "--swap"]

        def shards(tag):
            with contextlib.redirect_stdout(io.StringIO()) as out:
                expert.main(base + ["--shards", os.path.join(d, tag, "chunk"), "--desired-size", str(desired), "--files-per-chunk", "4"])
            return json.loads(out.getvalue().strip().splitlines()[-1])

        def log(tag):
            with contextlib.redirect_stdout(io.StringIO()):
                expert.main(base + ["--out", os.path.join(d, tag)])
            t1 = clock()
            per_map = db.split_by_map(os.path.join(d, tag, "PIBT.json"), os.path.join(d, tag, "temp"))
            t2 = clock()
            os.makedirs(os.path.join(d, tag, "shards"))
            rep = db.build_shards(named, named, [os.path.join(d, tag, "temp", f"{n}.json") for n in per_map], os.path.join(d, tag, "shards", "chunk"),
                                  desired, files_per_chunk=4)
            return t1, t2, rep, os.path.getsize(os.path.join(d, tag, "PIBT.json"))

        shards("warm")
        t0 = clock()
        line = shards("dev")
        t_dev = clock() - t0
        t0 = clock()
        t1, t2, rep, json_bytes = log("log")
        t3 = clock()
        fa = sorted(glob.glob(os.path.join(d, "dev", "chunk_part_*.arrow")))
        fb = sorted(glob.glob(os.path.join(d, "log", "shards", "chunk_part_*.arrow")))
        same = len(fa) == len(fb) == 4 and all(open(x, "rb").read() == open(y, "rb").read() for x, y in zip(fa, fb))
    return {"tool": "bench_episode_rows", "mode": "e2e", "maps": 4, "episodes": line["episodes"], "solved": line["solved"], "rows": line["rows"],
            "rows_written": rep[0]["rows"], "files_equal": bool(same), "log_json_bytes": json_bytes,
            "shards_route_s": round(t_dev, 3),
            "log_route_s": {"total": round(t3 - t0, 3), "expert_out": round(t1 - t0, 3), "split_by_map": round(t2 - t1, 3),
                            "build_shards": round(t3 - t2, 3)},
            "speedup": round((t3 - t0) / t_dev, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["rows", "e2e"], required=True)
    ap.add_argument("--seeds", type=int, default=0, help="seeds per agent count (rows: 100; e2e: 8)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--lifelong", action="store_true", help="--mode rows on a lifelong expert: lifelong_rows against records() -> the generator")
    ap.add_argument("--out", default=None, help="default: profiles/bench_episode_rows.jsonl (bench_episode_rows_lifelong.jsonl with --lifelong)")
    a = ap.parse_args()
    if a.lifelong and a.mode != "rows":
        ap.error("--lifelong is a --mode rows run")
    a.out = a.out or os.path.join(ROOT, "profiles", "bench_episode_rows_lifelong.jsonl" if a.lifelong else "bench_episode_rows.jsonl")
    a.seeds = a.seeds or (100 if a.mode == "rows" else 8)
    rec = bench_rows(a) if a.mode == "rows" else bench_e2e(a)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
