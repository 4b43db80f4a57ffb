"""Delta data generation: roll the policy out, find the state of each episode from which the expert's cost-to-go
jumped the most, and let the expert label the episode from there -- the data the reference's fourth checkpoint (MAPF-GPT-DDG-2M.pt) was
fine-tuned on.  The generator is not in the reference; what runs here is this project's own restatement of the rule.

    run = BatchedRunner(..., record=True); run.reset(pos, goal); run.run(max_steps)
    out = ddg.collect(run, grids, goal, run_keys)            # out["records"]: toolbox records with algorithm "DDG"

    python -m mapf_gpt_amd.ddg --weights CKPT --config CONFIG.yaml [--maps MAPS.yaml] --out DIR
        [--every 16 --max-iters 1024 --refine-rounds 8 --shield pibt --precision P --seed 0]       # writes DIR/DDG.json
    python -m mapf_gpt_amd.ddg ... --shards PREFIX --desired-size N [--maze-ratio --files-per-chunk --num-chunks --shard-seed]

Per policy batch (on_target "nothing" only: a lifelong episode has no joint goal, hence no cost-to-go), with K = `every`, T the recorded
steps and J = T // K + 1:

  snapshots  snapshot j of instance i = the recorded positions at t_j = j * K; valid iff t_j <= lengths[i].
  probe      every valid (i, j) is one instance of BatchedExpert(**probe) on instance i's grid, reset at (snapshot, goal[i]) and run for
             probe_steps; its global id is g * J + j (g = the run's global index), so its draws do not depend on how the batch is cut
             into contexts.  solved = CSR == 1; cost c = the env's SoC if solved, else n_agents * (probe_steps + 1), strictly above any
             solved cost.  A snapshot with every agent on its goal costs 0 without a run.
  pick       candidates j: j and j + 1 valid and solved[i][j]; delta = c[j + 1] - c[j]; j* = the smallest j that maximises delta; the
             instance is picked iff it has a candidate and (min_delta is None or delta[j*] >= min_delta).  Integer arithmetic on the device.
  teacher    the picked states run as BatchedExpert(**teacher) episodes from (snapshot j*, goal) for teacher_steps with global id g; their
             records have algorithm "DDG" and env_grid_search = the run's key + ddg_step = t_j* + ddg_delta.  Unsolved ones stay in the
             file with CSR 0: the dataset tokenizer drops them as it drops any other.

DIR/DDG.json is what dataset_build.split_by_map and `dataset_build --logs` take where the reference has LaCAM.json; the loop is
ddg -> split_by_map -> dataset_build -> `training --init CKPT --dropout 0.1`.  The CLI prints one JSON line: episodes, snapshots probed,
picked, teacher_solved, rows (dataset rows of the solved teacher episodes), delta_mean / delta_max of the picks, seconds per stage.

With --shards the teacher's episodes go from its device log straight to .arrow shards (dataset_build.EpisodeStore /
build_shards_from_store): no DDG.json between the teacher and training unless --out asks for it too; the line
gains `chunks`, the chunk reports.  collect_from_trajectory(rows=True) hands the same rows back as device tensors.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

PROBE = dict(swap=True)
TEACHER = dict(search="lacam", swap=True, max_iters=1024, refine_rounds=8)
INT64_MIN = -(2 ** 63)


# ---- the arithmetic (any device; tests/test_ddg_cpu.py runs it on the host) ------------------------------------------------------
def n_snapshots(T, every):
    return int(T) // int(every) + 1


def snapshot_valid(lengths, T, every):
    """bool [n_inst, J]: snapshot j (at t_j = j * every) lies inside the episode, t_j <= lengths[i]."""
    t = torch.arange(n_snapshots(T, every), device=lengths.device, dtype=torch.int64) * int(every)
    return t[None, :] <= lengths.to(torch.int64)[:, None]


def unsolved_cost(n_agents, probe_steps):
    """The cost of a snapshot the probe did not solve: above n_agents * probe_steps, the largest sum of costs of a solved one."""
    return int(n_agents) * (int(probe_steps) + 1)


def pick(valid, solved, cost, min_delta=None):
    """valid, solved bool [n_inst, J], cost int64 [n_inst, J] -> (picked bool [n_inst], j* int64 [n_inst], delta* int64 [n_inst],
    delta int64 [n_inst, J - 1], cand bool [n_inst, J - 1]); j* and delta* are 0 where nothing is picked."""
    cost = cost.to(torch.int64)
    n, J = valid.shape
    if J < 2:
        z = torch.zeros((n,), dtype=torch.int64, device=valid.device)
        e = torch.zeros((n, 0), dtype=torch.int64, device=valid.device)
        return z.bool(), z, z.clone(), e, e.bool()
    cand = valid[:, :-1] & valid[:, 1:] & solved[:, :-1]
    delta = cost[:, 1:] - cost[:, :-1]
    masked = torch.where(cand, delta, torch.full_like(delta, INT64_MIN))
    best = masked.max(dim=1).values
    j_all = torch.arange(J - 1, device=valid.device, dtype=torch.int64)[None, :].expand(n, J - 1)
    first = torch.where(cand & (masked == best[:, None]), j_all, torch.full_like(j_all, J)).min(dim=1).values
    picked = cand.any(dim=1)
    if min_delta is not None:
        picked = picked & (best >= int(min_delta))
    zero = torch.zeros_like(best)
    return picked, torch.where(picked, first, zero), torch.where(picked, best, zero), delta, cand


def segments(ids, max_instances):
    """Cut the ascending list of global ids into (start, stop) index ranges of consecutive ids, at most max_instances long: each range
    runs as one expert context with inst_offset = its first id, so every instance plans under its own global id however the list is cut."""
    out, a = [], 0
    ids = [int(v) for v in ids]
    for k in range(1, len(ids) + 1):
        if k == len(ids) or ids[k] != ids[k - 1] + 1 or k - a >= int(max_instances):
            out.append((a, k))
            a = k
    return out


# ---- the device stages -------------------------------------------------------------------------------------------------------------
def _run_expert(grids, grid_of, ids, pos, goal, steps, kw, seed, max_instances, device, keys=None, algorithm=None, rows=None, store=None):
    """One expert episode per entry: entry e plans on grids[grid_of[e]] under global id ids[e] from (pos[e], goal[e]).
    -> (metrics float32 [n, 6] device tensor, records or None).  rows: a list that receives every entry's (rows, labels) device
    tensors (empty ones for an unsolved episode), from the expert's device log; store: an EpisodeStore that takes every context's log."""
    from .expert import BatchedExpert
    grids = np.asarray(grids)
    if grids.ndim == 2:
        grids = grids[None]
    metrics, records = [], []
    for a, b in segments(ids, max_instances):
        g = grids if len(grids) == 1 else np.stack([grids[int(k)] for k in grid_of[a:b]])
        ex = BatchedExpert(g, b - a, int(pos.shape[1]), int(steps), seed=seed, device=device, inst_offset=int(ids[a]), **kw)
        ex.reset(pos[a:b], goal[a:b])
        ex.run(int(steps))
        metrics.append(ex.metrics())
        if keys is not None:
            records.extend(ex.records(keys[a:b], pos[a:b], algorithm=algorithm))
        if rows is not None:
            per = [None] * (b - a)
            for inst, x, y, row0 in ex.dataset_rows(pos[a:b], tables=store.tables if store is not None else None, offsets=True):
                r0 = row0.cpu().tolist()
                for k, i in enumerate(inst):
                    per[int(i)] = (x[r0[k]:r0[k + 1]], y[r0[k]:r0[k + 1]])
            rows.extend(per)
        if store is not None:
            log, lens = ex.log()
            store.add_batch(keys[a:b], pos[a:b], log, lens, metrics[-1][:, 0] >= 1, g)
    n = len(ids)
    m = torch.cat(metrics) if metrics else torch.zeros((0, 6), dtype=torch.float32, device=device)
    assert m.shape[0] == n
    return m, (records if keys is not None else None)


def collect_from_trajectory(grids, pos_traj, lengths, goal, run_keys, every=16, probe=None, teacher=None, probe_steps=None,
                            teacher_steps=None, min_delta=None, seed=0, max_teacher_instances=4096, global_ids=None,
                            max_episode_steps=None, on_target="nothing", device="cuda", rows=False, store=None):
    """Probe, pick and teacher on a recorded batch.  grids [n_grids, H, W] (instance i lives on grid i % n_grids, as in BatchedRunner),
    pos_traj integer [T + 1, n_inst, n_agents, 2] and lengths [n_inst] as BatchedRunner.trajectory() gives them (tensors or arrays),
    goal [n_inst, n_agents, 2], run_keys: the env_grid_search dict of every instance; global_ids: every instance's g (default 0, 1, ..).
    probe_steps / teacher_steps default to max_episode_steps, and that to T.
    -> dict: records (the teacher's, in instance order), valid / solved / cost [n_inst, J], delta / cand [n_inst, J - 1], picked, j, dmax
    [n_inst] (numpy), teacher_metrics float32 [picked, 6], probed (snapshots run), seconds {probe, pick, teacher}.
    rows=True: the dict also has `rows` uint8 [N, 256] and `labels` int8 [N], device tensors: the rows of the solved teacher episodes in
    record order, from the teacher's device log (what the dataset tokenizer makes of `records`).  store: a dataset_build.EpisodeStore
    that takes the teacher's logs, one batch per expert context, in global-id order (= record order when global_ids ascend)."""
    if on_target != "nothing":
        raise NotImplementedError(f"on_target={on_target!r}: delta data needs a cost-to-go, and a lifelong episode has no joint goal to "
                                  "measure one against")
    dev = torch.device(device)
    probe = dict(PROBE if probe is None else probe)
    teacher = dict(TEACHER if teacher is None else teacher)
    pos_traj = torch.as_tensor(pos_traj).to(dev)
    lengths = torch.as_tensor(lengths).to(dev).to(torch.int64)
    goal = torch.as_tensor(goal).to(dev).to(torch.int16)
    T, n_inst, n_agents = int(pos_traj.shape[0]) - 1, int(pos_traj.shape[1]), int(pos_traj.shape[2])
    K = int(every)
    if K < 1:
        raise ValueError("every must be >= 1")
    J = n_snapshots(T, K)
    cap = int(max_episode_steps or T)
    probe_steps, teacher_steps = int(probe_steps or cap), int(teacher_steps or cap)
    gids = np.arange(n_inst, dtype=np.int64) if global_ids is None else np.asarray(global_ids, dtype=np.int64)
    assert len(gids) == n_inst == len(run_keys)
    n_grids = 1 if np.asarray(grids).ndim == 2 else len(grids)

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        return time.perf_counter()

    # probe: snapshots [n_inst, J, n_agents, 2], indexed on the device
    t0 = sync()
    snaps = pos_traj[0:T + 1:K].to(torch.int16).permute(1, 0, 2, 3).contiguous()
    valid = snapshot_valid(lengths, T, K)
    at_goal = (snaps == goal[:, None]).all(dim=3).all(dim=2)
    run_mask = valid & ~at_goal
    ii, jj = torch.nonzero(run_mask, as_tuple=True)                     # row-major: instance-major, j ascending
    ii_h, jj_h = ii.cpu().numpy(), jj.cpu().numpy()
    ids = gids[ii_h] * J + jj_h
    order = np.argsort(ids, kind="stable")                              # (global ids ascending: instance order wherever g is)
    ii_h, jj_h, ids = ii_h[order], jj_h[order], ids[order]
    sel_i, sel_j = torch.as_tensor(ii_h, device=dev), torch.as_tensor(jj_h, device=dev)
    m, _ = _run_expert(grids, ii_h % n_grids, ids, snaps[sel_i, sel_j], goal[sel_i], probe_steps, probe, seed, max_teacher_instances, dev)
    solved = valid & at_goal
    cost = torch.where(valid, torch.full((n_inst, J), unsolved_cost(n_agents, probe_steps), dtype=torch.int64, device=dev),
                       torch.zeros((n_inst, J), dtype=torch.int64, device=dev))
    cost = torch.where(at_goal, torch.zeros_like(cost), cost)
    if len(ids):
        ok = m[:, 0] >= 1.0
        solved[sel_i, sel_j] = ok
        cost[sel_i, sel_j] = torch.where(ok, m[:, 2].to(torch.int64), cost[sel_i, sel_j])
    t1 = sync()

    picked, jstar, dmax, delta, cand = pick(valid, solved, cost, min_delta)
    t2 = sync()

    # teacher: the picked states under global id g
    p_h = torch.nonzero(picked).view(-1).cpu().numpy()
    p_h = p_h[np.argsort(gids[p_h], kind="stable")]
    j_h, d_h = jstar.cpu().numpy(), dmax.cpu().numpy()
    keys = []
    for i in p_h:
        key = dict(run_keys[int(i)])
        key["ddg_step"], key["ddg_delta"] = int(j_h[i]) * K, int(d_h[i])
        keys.append(key)
    sel = torch.as_tensor(p_h, device=dev)
    ep_rows = [] if rows else None
    tm, records = _run_expert(grids, p_h % n_grids, gids[p_h], snaps[sel, jstar[sel]], goal[sel], teacher_steps, teacher, seed,
                              max_teacher_instances, dev, keys=keys, algorithm="DDG", rows=ep_rows, store=store)
    back = np.argsort(p_h, kind="stable")                               # from global-id order back to instance order
    extra = {}
    if rows:
        xs = [ep_rows[k][0] for k in back] + [torch.empty((0, 256), dtype=torch.uint8, device=dev)]
        ys = [ep_rows[k][1] for k in back] + [torch.empty((0,), dtype=torch.int8, device=dev)]
        extra = {"rows": torch.cat(xs), "labels": torch.cat(ys)}
    t3 = sync()
    return {**extra, "records": [records[k] for k in back], "valid": valid.cpu().numpy(), "solved": solved.cpu().numpy(), "cost": cost.cpu().numpy(),
            "delta": delta.cpu().numpy(), "cand": cand.cpu().numpy(), "picked": picked.cpu().numpy(), "j": j_h, "dmax": d_h,
            "teacher_metrics": tm.cpu().numpy()[back], "probed": int(len(ids)), "every": K, "J": J,
            "seconds": {"probe": t1 - t0, "pick": t2 - t1, "teacher": t3 - t2}}


def collect(runner, grids, goal, run_keys, **kw):
    """collect_from_trajectory on a recording runner's own episode (BatchedRunner(record=True), after its run)."""
    if runner.env.lifelong:
        raise NotImplementedError("delta data needs a cost-to-go, and a lifelong (on_target='restart') episode has no joint goal to "
                                  "measure one against")
    pos, _, lengths = runner.trajectory()
    kw.setdefault("max_episode_steps", runner.env.max_episode_steps)
    kw.setdefault("device", runner.device)
    return collect_from_trajectory(grids, pos, lengths, goal, run_keys, **kw)


def dataset_rows(records):
    """Rows the dataset tokenizer makes of `records`: (ep_length + 1) x agents of every episode with CSR = 1."""
    return sum(len(r["metrics"]["made_actions"]) * (len(r["metrics"]["made_actions"][0]) + 1) for r in records if r["metrics"]["CSR"] >= 1)


def main(argv=None):
    ap = argparse.ArgumentParser(description="Roll a policy out over an evaluation config and write the expert's relabelled delta data to DIR/DDG.json")
    ap.add_argument("--weights", required=True, help="the policy's checkpoint (or synthetic:<shape>[:seed])")
    ap.add_argument("--config", required=True, help="evaluation YAML (its environment: block is run)")
    ap.add_argument("--maps", default=None, help="maps.yaml ({name: map string}) registered on top of the built-in maps")
    ap.add_argument("--out", default=None, help="output directory (optional with --shards)")
    ap.add_argument("--shards", default=None, metavar="PREFIX", help="write .arrow shards from the teacher's device log")
    ap.add_argument("--desired-size", type=int, default=None, help="--shards: rows per chunk")
    ap.add_argument("--maze-ratio", type=float, default=0.9)
    ap.add_argument("--files-per-chunk", type=int, default=10)
    ap.add_argument("--num-chunks", type=int, default=1)
    ap.add_argument("--shard-seed", type=int, default=0, help="--shards: seed of the shuffles (dataset_build --seed)")
    ap.add_argument("--every", type=int, default=16, help="steps between two snapshots")
    ap.add_argument("--max-iters", type=int, default=TEACHER["max_iters"], help="iterations of the teacher's search per instance")
    ap.add_argument("--refine-rounds", type=int, default=TEACHER["refine_rounds"], help="rounds of the teacher's refinement pass (0 = off)")
    ap.add_argument("--min-delta", type=int, default=None, help="pick an episode only if its largest delta reaches this")
    ap.add_argument("--shield", choices=["pibt"], default=None, help="roll the policy out behind the collision shield")
    ap.add_argument("--precision", default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    if a.shards is None and a.out is None:
        ap.error("one of --out and --shards is required")
    if a.shards is not None and a.desired_size is None:
        ap.error("--shards needs --desired-size")
    from . import evaluation as ev
    cfg = ev.load_yaml(a.config)
    reg = ev.MapRegistry()
    if a.maps:
        reg.register_maps(ev.load_yaml(a.maps))
    store = None
    if a.shards is not None:
        from .dataset_build import EpisodeStore, build_shards_from_store
        store = EpisodeStore(device=a.device)
    algo = {"name": "MAPF-GPT", "path_to_weights": a.weights, "seed": a.seed, "device": a.device}
    if a.shield:
        algo["shield"] = a.shield
    cfg = {"environment": cfg["environment"], "algorithms": {"MAPF-GPT": algo}}
    teacher = dict(TEACHER, max_iters=a.max_iters, refine_rounds=a.refine_rounds)
    if not a.refine_rounds:
        del teacher["refine_rounds"]
    records, deltas = [], []
    line = {"episodes": 0, "snapshots": 0, "picked": 0, "teacher_solved": 0, "rows": 0}
    secs = {"rollout": 0.0, "probe": 0.0, "pick": 0.0, "teacher": 0.0}

    def on_batch(info):
        out = collect(info["runner"], info["grids"], info["goal"], info["run_keys"], every=a.every, teacher=teacher, seed=a.seed,
                      global_ids=info["mine"], max_episode_steps=info["max_steps"], on_target=info["on_target"], store=store)
        records.extend(out["records"])
        deltas.extend(int(d) for d, p in zip(out["dmax"], out["picked"]) if p)
        line["snapshots"] += out["probed"]
        for k, v in out["seconds"].items():
            secs[k] += v

    t0 = time.perf_counter()
    res = ev.evaluation(cfg, registry=reg, precision=a.precision, print_fn=lambda *_: None, record=True, on_batch=on_batch)
    secs["rollout"] = time.perf_counter() - t0 - secs["probe"] - secs["pick"] - secs["teacher"]
    if a.out is not None:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "DDG.json"), "w") as f:
            json.dump(records, f, indent=1)
    line.update(episodes=len(res), picked=len(records), teacher_solved=sum(1 for r in records if r["metrics"]["CSR"] >= 1),
                rows=dataset_rows(records), delta_mean=round(float(np.mean(deltas)), 3) if deltas else 0.0,
                delta_max=max(deltas) if deltas else 0, seconds={k: round(v, 3) for k, v in secs.items()})
    if store is not None:
        t1 = time.perf_counter()
        if os.path.dirname(a.shards):
            os.makedirs(os.path.dirname(a.shards), exist_ok=True)
        line["chunks"] = build_shards_from_store(store, a.shards, a.desired_size, a.maze_ratio, a.files_per_chunk, a.num_chunks, a.shard_seed)
        line["seconds"]["shards"] = round(time.perf_counter() - t1, 3)
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
