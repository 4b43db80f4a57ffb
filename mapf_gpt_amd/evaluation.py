"""Evaluation harness: the role of the reference's `benchmark.py` + `pogema_toolbox.evaluator.evaluation`
(benchmark.py:20-50) for configs in the reference's YAML format (eval_configs/*/*.yaml + maps.yaml).

What the reference does per folder: register the maps, expand every `grid_search` list of the
`environment:` block into the cartesian product of runs, run every algorithm of `algorithms:` on every
run (one episode per worker process, dask pool of `num_process`), collect the episode metrics
(create_env.py:15-19: infos[0]["metrics"]) and render `results_views`.

Here all runs of one (algorithm, num_agents) group become instances of ONE device-resident batch
(`BatchedRunner`): maps are padded to a common frame (extra obstacle cells change nothing for the
agents), starts/goals are drawn per (map, seed), and the whole group steps together on the GPU.
With `torch.distributed` initialised the instances of a group are sharded over the ranks and the
metric records are gathered once (runner.gather_metrics).

Result records keep the toolbox's shape: {"metrics": {...}, "env_grid_search": {...}, "algorithm": name}.
Metric keys: CSR, ISR, SoC, makespan, ep_length (env spec: DESIGN.md section 4; `avg_throughput` for
on_target="restart" runs) and `runtime`
(seconds; the group's wall time divided by its instances -- a batched run has no per-episode clock).
Placement is this repo's seeded generator, not POGEMA's (absent offline): numbers are comparable to
the paper's only in distribution, not seed for seed.
"""
import itertools
import json
import os
import time
from collections import OrderedDict

import numpy as np

from . import maps as _maps

METRIC_KEYS = ("CSR", "ISR", "SoC", "makespan", "ep_length", "avg_agents_density")
LIFELONG_QUEUE = 64          # goals pre-generated per agent in on_target="restart" runs (the queue wraps)


# ---- config handling (pure python, testable without a GPU) -------------------------------------
def expand_grid_search(env_cfg):
    """`environment:` block -> list of (full_cfg, grid_point) in the product order of the keys as written."""
    keys = [k for k, v in env_cfg.items() if isinstance(v, dict) and "grid_search" in v]
    lists = [list(env_cfg[k]["grid_search"]) for k in keys]
    base = {k: v for k, v in env_cfg.items() if k not in keys}
    out = []
    for combo in itertools.product(*lists):
        point = OrderedDict(zip(keys, combo))
        cfg = dict(base)
        cfg.update(point)
        out.append((cfg, dict(point)))
    return out


def load_yaml(path):
    import yaml
    with open(path) as f:
        return yaml.safe_load(f)


class MapRegistry:
    """name -> map string; `register_maps` mirrors ToolboxRegistry.register_maps (benchmark.py:38-41)."""

    def __init__(self):
        self._maps = dict(_maps.named_maps())

    def register_maps(self, maps):
        self._maps.update(maps)

    def get(self, name):
        if name not in self._maps:
            raise KeyError(f"map '{name}' is not registered (register_maps(yaml of eval_configs/<folder>/maps.yaml))")
        return _maps.parse_map(self._maps[name])


def common_frame(parsed, r=_maps.OBS_RADIUS):
    """Pad every (obst, start_ok, goal_ok) to one (H, W): r obstacle cells on every side, then obstacle
    fill to the largest map (top-left aligned)."""
    H = max(p[0].shape[0] for p in parsed) + 2 * r
    W = max(p[0].shape[1] for p in parsed) + 2 * r
    out = []
    for obst, s_ok, g_ok in parsed:
        g = np.ones((H, W), np.uint8)
        s = np.zeros((H, W), bool)
        t = np.zeros((H, W), bool)
        h, w = obst.shape
        g[r:r + h, r:r + w] = obst
        s[r:r + h, r:r + w] = s_ok
        t[r:r + h, r:r + w] = g_ok
        out.append((g, s, t))
    return out


def lifelong_cells(frame):
    """The cells a lifelong queue draws from: those of the largest free component of frame = (grid, start_ok, goal_ok) that may be goals."""
    g, _, g_ok = frame
    return np.argwhere(_maps.largest_component(g == 0) & g_ok)


def lifelong_queue(frame, seed, n_agents, length=LIFELONG_QUEUE, cells=None):
    """The seeded queue of further goals of one on_target="restart" run: int16 [n_agents, length, 2] of lifelong_cells(frame) (`cells`:
    that array, where the caller seeds many runs on one frame)."""
    cells = lifelong_cells(frame) if cells is None else cells
    rng = np.random.Generator(np.random.PCG64([int(seed), 0x4C4C]))
    return cells[rng.integers(0, len(cells), (n_agents, length))].astype(np.int16)


def group_runs(runs):
    """Runs that can share one batch: same num_agents, max_episode_steps and on_target."""
    groups = OrderedDict()
    for i, (cfg, point) in enumerate(runs):
        key = (int(cfg["num_agents"]), int(cfg.get("max_episode_steps", 128)), cfg.get("on_target", "nothing"))
        groups.setdefault(key, []).append(i)
    return groups


def tabular_view(results, view_cfg, print_fn=print):
    """`type: tabular` of results_views: drop `drop_keys`, group by the remaining grid keys + algorithm, mean."""
    drop = set(view_cfg.get("drop_keys", []))
    digits = int(view_cfg.get("round_digits", 2))
    rows = OrderedDict()
    for r in results:
        key = tuple((k, v) for k, v in r["env_grid_search"].items() if k not in drop) + (("algorithm", r["algorithm"]),)
        rows.setdefault(key, []).append(r["metrics"])
    present = set().union(*[set(r["metrics"]) for r in results]) if results else set()
    cols = [k for k in list(METRIC_KEYS) + ["avg_throughput", "runtime"] if k not in drop and k in present]
    table = []
    for key, ms in rows.items():
        rec = OrderedDict(key)
        for c in cols:
            rec[c] = round(float(np.mean([m[c] for m in ms])), digits)
        table.append(rec)
    if table and view_cfg.get("print_results", False):
        hdr = list(table[0].keys())
        wid = [max(len(str(h)), max(len(str(t[h])) for t in table)) for h in hdr]
        print_fn("  ".join(str(h).ljust(w) for h, w in zip(hdr, wid)))
        for t in table:
            print_fn("  ".join(str(t[h]).ljust(w) for h, w in zip(hdr, wid)))
    return table


def plot_series(results, view_cfg):
    """Data of a `type: plot` view (eval_configs/01-random/01-random.yaml:162-186): per algorithm, the mean of metric
    `y` at every value of grid key `x` over all other grid keys (seeds, maps), with a normal-approximation 95 % interval
    of that mean -> {algorithm: [(x, mean, lo, hi, n), ...]} sorted by x."""
    xk, yk = view_cfg["x"], view_cfg["y"]
    acc = OrderedDict()
    for r in results:
        if xk not in r["env_grid_search"] or yk not in r["metrics"]:
            continue
        acc.setdefault(r["algorithm"], OrderedDict()).setdefault(r["env_grid_search"][xk], []).append(float(r["metrics"][yk]))
    out = OrderedDict()
    for algo, by_x in acc.items():
        pts = []
        for x in sorted(by_x):
            v = np.asarray(by_x[x], dtype=np.float64)
            half = 1.96 * v.std(ddof=1) / np.sqrt(len(v)) if len(v) > 1 else 0.0
            pts.append((x, float(v.mean()), float(v.mean() - half), float(v.mean() + half), len(v)))
        out[algo] = pts
    return out


def plot_view(results, view_cfg, path):
    """`type: plot` of results_views: one line per algorithm, metric `y` against grid key `x` with the interval band;
    honours width/height (inches), line_width, use_log_scale_x, ticks, font_size, legend_font_size, name (title).
    Writes `path` (format by extension) and returns the plotted series."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    series = plot_series(results, view_cfg)
    fs = view_cfg.get("font_size", 8)
    fig, ax = plt.subplots(figsize=(float(view_cfg.get("width", 3.0)), float(view_cfg.get("height", 2.5))))
    for algo, pts in series.items():
        xs = [p[0] for p in pts]
        line, = ax.plot(xs, [p[1] for p in pts], marker="o", markersize=3, linewidth=float(view_cfg.get("line_width", 2)), label=algo)
        ax.fill_between(xs, [p[2] for p in pts], [p[3] for p in pts], alpha=0.2, color=line.get_color(), linewidth=0)
    if view_cfg.get("use_log_scale_x", False):
        ax.set_xscale("log")
    if view_cfg.get("use_log_scale_y", False):
        ax.set_yscale("log")
    if view_cfg.get("ticks"):
        ax.set_xticks(list(view_cfg["ticks"]))
        ax.set_xticklabels([str(t) for t in view_cfg["ticks"]])
        ax.minorticks_off()
    ax.set_xlabel(str(view_cfg["x"]), fontsize=fs)
    ax.set_ylabel(str(view_cfg["y"]), fontsize=fs)
    ax.tick_params(labelsize=fs)
    if view_cfg.get("name"):
        ax.set_title(str(view_cfg["name"]), fontsize=fs)
    if series:
        ax.legend(fontsize=view_cfg.get("legend_font_size", fs))
    ax.grid(True, alpha=0.3)
    fig.tight_layout()
    fig.savefig(path)
    plt.close(fig)
    return series


# ---- the batched evaluation (GPU) -----------------------------------------------------------------
def _build_algorithm(algo_cfg, max_rows):
    from .inference import MAPFGPTInference, MAPFGPTInferenceConfig
    cfg = MAPFGPTInferenceConfig(**algo_cfg)                   # unknown keys raise, as in the reference (extra=forbid)
    cfg.batch_size = max(int(cfg.batch_size), 1)
    algo = MAPFGPTInference(cfg)
    return algo, cfg


class PIBTConfig:
    """Config of the `name: PIBT` algorithm (the device-resident expert, mapf_gpt_amd/expert.py): name, seed, device, swap (the
    corridor swap rule of DESIGN.md section 22, off by default), lifelong (plan the on_target: restart groups, DESIGN.md section 30, off
    by default); unknown keys raise, as for the MAPF-GPT config."""

    def __init__(self, name="PIBT", seed=0, device="cuda", swap=False, lifelong=False):
        self.name, self.seed, self.device, self.swap, self.lifelong = name, int(seed or 0), device, bool(swap), bool(lifelong)


class LaCAMConfig(PIBTConfig):
    """Config of the `name: LaCAM` algorithm: the same expert with a LaCAM search in front of every episode;
    name, seed, device, max_iters, swap, refine_rounds and refine_horizon (the refinement pass of section 26, off by default).
    `lifelong` is read and changes nothing: the search does not run on_target: restart groups."""

    def __init__(self, name="LaCAM", seed=0, device="cuda", max_iters=4096, swap=False, refine_rounds=0, refine_horizon=None, lifelong=False):
        super().__init__(name, seed, device, swap, lifelong)
        self.max_iters = int(max_iters)
        self.refine_rounds, self.refine_horizon = int(refine_rounds or 0), (int(refine_horizon) if refine_horizon else None)


def evaluation(evaluation_config, eval_dir=None, registry=None, precision=None, max_rows_per_batch=65536, rank=0, world=1,
               print_fn=print, trace=None, retire_done=False, log_actions=False, search_status=None, refine_stats=None, record=False,
               on_batch=None, on_expert_batch=None):
    """Run `evaluation_config` (dict in the reference's YAML schema).  Returns the list of result records (on every
    rank); writes `<eval_dir>/<algorithm>.json` and prints the tabular views on rank 0.
    `trace(kind, payload)` (tests): called with ("reset", {algorithm, runs, grids, pos, goal, max_steps}) for every batch
    this rank runs (plus on_target and goal_queue: the lifelong queues, else None) and with ("step", int32 actions [instances, agents])
    after every step -- the device's sampled actions, from which an episode can be replayed on the host.
    retire_done: BatchedRunner's retire mode -- finished episodes leave the policy's batch and a batch ends when none is live (the
    reference's run_episode leaves at all(terminated) or all(truncated), create_env.py:15-18); same records, less work.
    An algorithm whose `name` is PIBT runs the device-resident expert (BatchedExpert) instead of a policy: same grouping, frames,
    placement, sharding and metrics gather.  log_actions: the role of the reference's create_logging_env (create_env.py:8-33) -- the
    PIBT records also carry `made_actions` (per agent, cut to the episode's length) and `init_positions` (padded coordinates), the
    expert log that dataset_build / dataset_tokenizer consume; one rank only.  A PIBT entry with `lifelong: true` also runs the
    on_target="restart" groups (BatchedExpert(lifelong=True) on the seeded queue the policy branch gets; throughput in the ISR column as
    for a policy; with log_actions the records also carry `global_lifelong_targets_xy`); without it, and for LaCAM, such a group raises.
    An algorithm whose `name` is LaCAM is the same expert with search="lacam"; search_status (a dict) then receives the count of this rank's instances per (final) search status, and with
    `refine_rounds` in the entry refine_stats (a dict) receives `refined` (instances whose length or sum of costs fell), `rescued` (first
    status 4, final status 1) and `soc_before` / `soc_after` summed over the refined instances.
    A MAPF-GPT entry with `shield: pibt` runs its policy behind the collision shield (BatchedRunner(shield="pibt"));
    its records also carry `shield_overrides`: the agents whose planned action was not the sampled one, summed over the episode and
    divided by ep_length x num_agents.  Such an entry raises on an on_target="restart" group, as log_actions does, unless it also says
    `shield_lifelong: true`: its restart groups then run behind BatchedRunner(shield="pibt", shield_lifelong=True)
    on the seeded queue every policy entry gets, and their records carry `avg_throughput` and `shield_overrides`; its on_target="nothing"
    groups run the plain shield as before.
    record: MAPF-GPT entries run a recording runner (BatchedRunner(record=True)) and their records also carry
    `made_actions` (the actions the env was handed, cut to the episode's length), `init_positions` and `moves` (the actions the env
    executed); one rank only, as log_actions, which keeps its meaning (the expert's logs).  on_batch(info): called after each policy
    batch has run, info = {runner, algorithm, mine (the run indices of the batch, in instance order), grids, pos, goal, run_keys,
    n_agents, max_steps, on_target} -- how mapf_gpt_amd.ddg reads the recorded trajectories while they are on the device.
    on_expert_batch(info): the same for the PIBT / LaCAM batches, called after each has run, with `expert` (the BatchedExpert, its log
    and metrics still on the device) in the place of `runner` -- how dataset_build.EpisodeStore takes the episodes without a JSON log
    (DESIGN.md section 33).  on_batch keeps its meaning: policy batches only."""
    import torch
    from .runner import BatchedRunner, gather_metrics, shard_range

    if log_actions and world != 1:
        raise ValueError("log_actions=True needs world == 1: the action logs are not gathered across ranks")
    if record and world != 1:
        raise ValueError("record=True needs world == 1: the recorded episodes are not gathered across ranks")

    registry = registry or MapRegistry()
    runs = expand_grid_search(evaluation_config["environment"])
    groups = group_runs(runs)
    results = []
    for algo_name, algo_cfg in evaluation_config["algorithms"].items():
        algo_cfg = dict(algo_cfg)
        is_pibt = algo_cfg.get("name") in ("PIBT", "LaCAM")
        if is_pibt:
            algo, cfg = None, (LaCAMConfig if algo_cfg.get("name") == "LaCAM" else PIBTConfig)(**algo_cfg)
        else:
            if precision is not None:
                algo_cfg["precision"] = precision
            algo, cfg = _build_algorithm(algo_cfg, max_rows_per_batch)
        for (n_agents, max_steps, on_target), idxs in groups.items():
            if on_target not in ("nothing", "restart"):
                raise NotImplementedError(f"on_target={on_target!r}: 'nothing' and 'restart' (lifelong) are built")
            if is_pibt and on_target == "restart" and isinstance(cfg, LaCAMConfig):
                raise NotImplementedError("the LaCAM search does not plan lifelong (on_target='restart') episodes: it looks for a joint "
                                          "goal configuration (a PIBT entry with lifelong: true does)")
            if is_pibt and on_target == "restart" and not cfg.lifelong:
                raise NotImplementedError("the PIBT expert does not plan lifelong (on_target='restart') episodes unless its entry says "
                                          "lifelong: true")
            shield = None if is_pibt else getattr(cfg, "shield", None)
            shield_lifelong = bool(shield) and on_target == "restart" and bool(getattr(cfg, "shield_lifelong", False))
            if shield and on_target == "restart" and not shield_lifelong:
                raise NotImplementedError("shield: pibt does not plan lifelong (on_target='restart') episodes")
            parsed = [registry.get(runs[i][0]["map_name"]) for i in idxs]
            frames = dict(zip(idxs, common_frame(parsed)))
            per_batch = max(1, max_rows_per_batch // n_agents)
            for b0 in range(0, len(idxs), per_batch):
                chunk = idxs[b0:b0 + per_batch]
                lo, hi = shard_range(len(chunk), rank, world)
                mine = chunk[lo:hi]
                local = torch.zeros((0, len(METRIC_KEYS) + (1 if shield else 0)), dtype=torch.float32, device=cfg.device)
                t0 = time.perf_counter()
                logged, recorded = {}, {}
                if mine:
                    grids = np.stack([frames[i][0] for i in mine])
                    pos = np.empty((len(mine), n_agents, 2), np.int16)
                    goal = np.empty((len(mine), n_agents, 2), np.int16)
                    for k, i in enumerate(mine):
                        g, s_ok, g_ok = frames[i]
                        pos[k], goal[k] = _maps.place_agents(g, n_agents, int(runs[i][0].get("seed", 0)), s_ok, g_ok)
                    if is_pibt:
                        from .expert import BatchedExpert
                        search = {}
                        if isinstance(cfg, LaCAMConfig):
                            search = dict(search="lacam", max_iters=cfg.max_iters, refine_rounds=cfg.refine_rounds,
                                          refine_horizon=cfg.refine_horizon)
                        run = BatchedExpert(grids, len(mine), n_agents, max_steps, seed=cfg.seed, device=cfg.device, inst_offset=lo,
                                            swap=cfg.swap, lifelong=on_target == "restart", **search)
                    else:
                        run = BatchedRunner(grids, len(mine), n_agents, algo.net, max_episode_steps=max_steps,
                                            seed=int(cfg.seed or 0), do_sample=True, precision=cfg.precision, device=cfg.device,
                                            row_offset=lo * n_agents, retire_done=bool(retire_done), **({"shield": shield} if shield else {}),
                                            **({"shield_lifelong": True} if shield_lifelong else {}), **({"record": True} if record else {}))
                    queue = None
                    if on_target == "restart":          # lifelong: a seeded queue of further goals per agent (wraps)
                        queue = np.empty((len(mine), n_agents, LIFELONG_QUEUE, 2), np.int16)
                        for k, i in enumerate(mine):
                            queue[k] = lifelong_queue(frames[i], runs[i][0].get("seed", 0), n_agents)
                        queue = torch.from_numpy(queue)
                    if is_pibt:
                        run.reset(torch.from_numpy(pos), torch.from_numpy(goal), goal_queue=queue)
                        if run.search and search_status is not None:
                            for v in run.search_stats()[0].cpu().tolist():
                                search_status[v] = search_status.get(v, 0) + 1
                        if run.search and run.refine_rounds and refine_stats is not None:
                            final, _, _, length = (x.cpu().numpy() for x in run.search_stats())
                            first, first_len, soc0, soc1, _, _ = (x.cpu().numpy() for x in run.refine_stats())
                            better = (length < first_len) | (soc1 < soc0)
                            for k, v in (("refined", better.sum()), ("rescued", ((first == 4) & (final == 1)).sum()),
                                         ("soc_before", soc0[better].sum()), ("soc_after", soc1[better].sum())):
                                refine_stats[k] = refine_stats.get(k, 0) + int(v)
                    else:
                        run.reset(torch.from_numpy(pos), torch.from_numpy(goal), goal_queue=queue)
                    if trace is None:
                        run.run(max_steps)
                    else:
                        trace("reset", {"algorithm": algo_name, "runs": list(mine), "grids": grids.copy(), "pos": pos.copy(),
                                        "goal": goal.copy(), "max_steps": max_steps, "on_target": on_target,
                                        "goal_queue": None if queue is None else queue.numpy().copy()})
                        for _ in range(max_steps):
                            run.step()
                            trace("step", run.actions.cpu().numpy().copy())
                    local = run.metrics().to(torch.float32)
                    if queue is not None:               # ISR column carries the throughput (arrivals per step) in lifelong runs
                        local[:, 1] = run.throughput() if is_pibt else run.env.goals_reached().sum(1).to(torch.float32) / float(max_steps)
                    if shield:                          # one more column for the gather: the episode's override count
                        local = torch.cat([local, run.shield_overrides().to(torch.float32)[:, None]], dim=1)
                    if is_pibt and log_actions:
                        logged = dict(zip(mine, run.made_actions()))
                        init = dict(zip(mine, pos.tolist()))
                        if queue is not None:
                            targets = dict(zip(mine, run.targets()))
                    if not is_pibt and record:
                        recorded = dict(zip(mine, (r["metrics"] for r in run.records([runs[i][1] for i in mine], algo_name))))
                    if is_pibt and on_expert_batch is not None:
                        on_expert_batch({"expert": run, "algorithm": algo_name, "mine": list(mine), "grids": grids, "pos": pos, "goal": goal,
                                         "run_keys": [runs[i][1] for i in mine], "n_agents": n_agents, "max_steps": max_steps,
                                         "on_target": on_target})
                    if not is_pibt and on_batch is not None:
                        on_batch({"runner": run, "algorithm": algo_name, "mine": list(mine), "grids": grids, "pos": pos, "goal": goal,
                                  "run_keys": [runs[i][1] for i in mine], "n_agents": n_agents, "max_steps": max_steps,
                                  "on_target": on_target})
                    torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                allm = gather_metrics(local, len(chunk), rank, world).cpu().numpy()
                for k, i in enumerate(chunk):
                    m = {key: float(allm[k, j]) for j, key in enumerate(METRIC_KEYS)}
                    if on_target == "restart":
                        m = {"avg_throughput": m["ISR"], "ep_length": m["ep_length"]}
                    if shield:
                        m["shield_overrides"] = float(allm[k, len(METRIC_KEYS)]) / max(1.0, m["ep_length"] * n_agents)
                    m["runtime"] = dt / max(1, len(chunk))
                    if i in logged:
                        m["made_actions"], m["init_positions"] = logged[i], init[i]
                        if on_target == "restart":
                            m["global_lifelong_targets_xy"] = targets[i]
                    if i in recorded:
                        m.update({key: recorded[i][key] for key in ("made_actions", "init_positions", "moves")})
                    results.append({"metrics": m, "env_grid_search": runs[i][1], "algorithm": algo_name})
        del algo
    if rank == 0:
        if eval_dir is not None:
            os.makedirs(eval_dir, exist_ok=True)
            for algo_name in evaluation_config["algorithms"]:
                with open(os.path.join(eval_dir, f"{algo_name}.json"), "w") as f:
                    json.dump([r for r in results if r["algorithm"] == algo_name], f, indent=1)
        for view_name, view in (evaluation_config.get("results_views") or {}).items():
            if view.get("type") == "tabular":
                print_fn(f"== {view_name}")
                tabular_view(results, view, print_fn)
            elif view.get("type") == "plot" and eval_dir is not None:
                plot_view(results, view, os.path.join(eval_dir, f"{view_name}.pdf"))
    return results


def run_folder(folder, eval_root="eval_configs", **kw):
    """= one iteration of benchmark.py:37-50 on a folder laid out like the reference's eval_configs/<folder>/."""
    reg = MapRegistry()
    maps_path = os.path.join(eval_root, folder, "maps.yaml")
    if os.path.exists(maps_path):
        reg.register_maps(load_yaml(maps_path))
    cfg = load_yaml(os.path.join(eval_root, folder, f"{os.path.basename(folder)}.yaml"))
    return evaluation(cfg, eval_dir=os.path.join(eval_root, folder), registry=reg, **kw)
