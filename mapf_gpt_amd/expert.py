"""Device-resident PIBT expert: the role of the reference's `run_expert()` (dataset/generate_dataset.py:214-230) with its logging
environment (experiment_setup/create_env.py:8-33, 49-60) -- step 1 of the dataset pipeline, and a baseline for the evaluation tables.

The reference's expert is LaCAM3 under POGEMA; neither is in its tree.  What runs here is PIBT (priority inheritance with
backtracking), the configuration generator of such a search, by this project's own spec, one wave64 workgroup per
instance on the BFS distance fields the tokenizer keeps in HBM.  It is a WEAKER teacher than LaCAM: nothing guarantees that all agents
stand on their goals at once, and episodes that do not end with CSR = 1 are dropped by the dataset tokenizer as the reference drops them.

    ex = BatchedExpert(grids, n_inst, n_agents, max_episode_steps, seed=0)
    ex.reset(pos, goal); ex.run(max_episode_steps)
    records = ex.records(run_keys, pos)            # toolbox records with made_actions / init_positions

    python -m mapf_gpt_amd.expert --config CONFIG.yaml --maps MAPS.yaml --out DIR      # writes DIR/PIBT.json
    python -m mapf_gpt_amd.expert --algo lacam [--max-iters N] ...                      # writes DIR/LaCAM.json
    python -m mapf_gpt_amd.expert [--algo lacam] --swap ...                             # the same files, with the corridor swap rule
    python -m mapf_gpt_amd.expert --algo lacam --refine-rounds N [--refine-horizon H]   # ... with found solutions refined

`search="lacam"` puts a LaCAM search (plain depth-first LaCAM over this PIBT as its configuration generator) in
front of the episode: reset() solves every instance on the device, an instance solved within the step cap replays its solution, every
other instance is planned step by step by PIBT as before, so the expert is never worse than PIBT alone.

`swap=True` turns on the corridor swap rule in the generator, both in the episode's plan kernel and inside the
search: two agents that meet head-on in a corridor walk together to the nearest junction and exchange there.  Off by default; with it
off every result is bit for bit what it was.

`refine_rounds=N` (search mode only) refines every found solution of up to `refine_horizon` steps before the episode (DESIGN.md section
26): rounds in which every agent is replanned once, alone, against the others' fixed paths, until a round changes nothing or N rounds
have run.  No agent's arrival ever grows, so a solution longer than the step cap may come under it and is then replayed.  Off by default.

The config is an evaluation YAML (eval_configs/<folder>/<folder>.yaml): its `environment:` block is run; its `algorithms:` block is
replaced by one PIBT entry (seed from --seed).  DIR/PIBT.json is what `dataset_build.split_by_map` and `dataset_build --logs` take
where the reference has LaCAM.json.  Prints one JSON line: episodes, solved, rows, seconds (with --algo lacam also `status`: the
count of instances per search status; with --swap also `"swap": true`; with --refine-rounds also `refine_rounds`, `refined`: instances
whose length or sum of costs fell, `rescued`: instances the search left over the step cap that are now replayed, and `soc_before` /
`soc_after`: the sum of costs summed over the refined instances).
"""
import argparse
import ctypes
import json
import sys
import time

import numpy as np
import torch

from . import _lib
from .env import METRIC_KEYS, BatchedEnv
from .observation_generator import BatchedTokenizer


class BatchedExpert:
    """Same shape as BatchedRunner: owns a BatchedEnv and a BatchedTokenizer (used for its BFS distance fields only)."""

    def __init__(self, grids, n_inst, n_agents, max_episode_steps, seed=0, device="cuda", inst_offset=0, search=None, max_iters=4096,
                 iters_per_launch=None, hash_bits=0, swap=False, refine_rounds=0, refine_horizon=None):
        if search not in (None, "lacam"):
            raise ValueError(f"search={search!r}: None or 'lacam'")
        if refine_rounds and not search:
            raise ValueError("refine_rounds needs search='lacam': the pass refines what the search found")
        self.device = torch.device(device)
        self.env = BatchedEnv(grids, n_inst, n_agents, max_episode_steps, device=device)
        self.tok = BatchedTokenizer(grids, n_inst, n_agents, device=device)
        self.n_inst, self.n_agents, self.max_episode_steps = int(n_inst), int(n_agents), int(max_episode_steps)
        self.seed, self.inst_offset = int(seed), int(inst_offset)
        self.actions = torch.zeros((n_inst, n_agents), dtype=torch.int32, device=self.device)
        self.t = 0
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mgpt_expert_create(ctypes.byref(self._h), self.tok._h, self.env._h, self.seed & (2 ** 64 - 1),
                                                     self.inst_offset, self.max_episode_steps))
        self.search, self.max_iters = search, int(max_iters)
        if search:           # iters_per_launch None = the library's default slice; hash_bits 0 = the table's own size (tests cut it short)
            with _lib.on_device(self.device):
                _lib.check(_lib.lib().mgpt_expert_set_search(self._h, self.max_iters, int(iters_per_launch or 0), int(hash_bits)))
        self.swap = False
        if swap:
            self.set_swap(True)
        self.refine_rounds = 0
        if refine_rounds:
            self.set_refine(refine_rounds, refine_horizon)

    def set_swap(self, on):
        """Turn the corridor swap rule on or off: before reset() or between episodes (MGPTError with ERR_STATE in the middle of one)."""
        with _lib.on_device(self.device):
            _lib.check(_lib.lib().mgpt_expert_set_swap(self._h, 1 if on else 0))
        self.swap = bool(on)

    def set_refine(self, max_rounds, horizon=None):
        """Turn the refinement pass of reset() on (max_rounds >= 1; horizon None = twice max_episode_steps) or off (0): before reset()
        or between episodes, in search mode only (MGPTError with ERR_STATE otherwise)."""
        with _lib.on_device(self.device):
            _lib.check(_lib.lib().mgpt_expert_set_refine(self._h, int(max_rounds), int(horizon or 0)))
        self.refine_rounds = int(max_rounds)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                _lib.lib().mgpt_expert_destroy(h)
            except Exception:      # interpreter shutdown
                pass
            self._h = None

    def reset(self, pos, goal):
        self.env.reset(pos, goal)
        self.tok.create_agents(self.env.pos, self.env.goal)       # the BFS distance-to-goal fields the planner reads
        self.actions.zero_()
        self.t = 0
        with _lib.on_device(self.device):
            _lib.check(_lib.lib().mgpt_expert_reset(self._h, _lib.stream_ptr()))
            if self.search:
                _lib.check(_lib.lib().mgpt_expert_solve(self._h, _lib.stream_ptr()))

    def search_stats(self):
        """-> status, iterations, nodes, solution length: int32 [n_inst] device tensors.  status 1 solved within the step cap (the
        instance replays its solution), 2 no solution exists, 3 max_iters reached, 4 solved but longer than the step cap."""
        out = [torch.empty((self.n_inst,), dtype=torch.int32, device=self.device) for _ in range(4)]
        with _lib.on_device(self.device):
            _lib.check(_lib.lib().mgpt_expert_copy_search(self._h, *[_lib.ptr(t) for t in out], _lib.stream_ptr()))
        return tuple(out)

    def refine_stats(self):
        """-> the search's own status and length, sum of costs before and after, rounds run, replans adopted: int32 [n_inst] device
        tensors (the last four are 0 for an instance the pass left as it is).  With the pass on, search_stats() and solution() report
        the final status, length and solution, which are what the episode replays."""
        out = [torch.empty((self.n_inst,), dtype=torch.int32, device=self.device) for _ in range(6)]
        with _lib.on_device(self.device):
            _lib.check(_lib.lib().mgpt_expert_copy_refine(self._h, *[_lib.ptr(t) for t in out], _lib.stream_ptr()))
        return tuple(out)

    def solution(self):
        """int8 [n_inst, n_agents, T]: the actions of the status-1 instances, 0 elsewhere (device tensor)."""
        out = torch.empty((self.n_inst, self.n_agents, self.max_episode_steps), dtype=torch.int8, device=self.device)
        with _lib.on_device(self.device):
            _lib.check(_lib.lib().mgpt_expert_copy_solution(self._h, _lib.ptr(out), _lib.stream_ptr()))
        return out

    def step(self):
        """plan -> log -> env.step -> since update in ONE library call (mgpt_expert_step)."""
        with _lib.on_device(self.device):
            _lib.check(_lib.lib().mgpt_expert_step(self._h, _lib.ptr(self.actions.view(-1)), _lib.stream_ptr()))
        self.t += 1

    def run(self, steps):
        for _ in range(steps):
            self.step()

    def metrics(self):
        return self.env.metrics()

    def planned(self):
        """int16 [n_inst, n_agents, 2]: the cell every agent planned to stand on after the last step (device tensor)."""
        out = torch.empty((self.n_inst, self.n_agents, 2), dtype=torch.int16, device=self.device)
        with _lib.on_device(self.device):
            _lib.check(_lib.lib().mgpt_expert_copy_plan(self._h, _lib.ptr(out), _lib.stream_ptr()))
        return out

    def log(self):
        """-> (made_actions int8 [n_inst, n_agents, T], lengths int32 [n_inst]) device tensors; T = max_episode_steps, an instance's
        entries beyond its length are 0."""
        log = torch.empty((self.n_inst, self.n_agents, self.max_episode_steps), dtype=torch.int8, device=self.device)
        lens = torch.empty((self.n_inst,), dtype=torch.int32, device=self.device)
        with _lib.on_device(self.device):
            _lib.check(_lib.lib().mgpt_expert_copy_log(self._h, _lib.ptr(log), _lib.ptr(lens), _lib.stream_ptr()))
        return log, lens

    def made_actions(self):
        """Per instance, per agent: the list of actions made, cut to the instance's episode length (host lists)."""
        log, lens = self.log()
        log, lens = log.cpu().numpy(), lens.cpu().numpy()
        return [[log[i, a, :int(lens[i])].tolist() for a in range(self.n_agents)] for i in range(self.n_inst)]

    def records(self, run_keys, init_pos, algorithm="PIBT"):
        """Toolbox result records (evaluation.py): metrics = the six env metrics + made_actions + init_positions (padded coordinates,
        as dataset_tokenizer.agent_paths expects), env_grid_search = run_keys[i], algorithm."""
        m = self.metrics().cpu().numpy()
        made = self.made_actions()
        init = np.asarray(init_pos.cpu() if torch.is_tensor(init_pos) else init_pos).reshape(self.n_inst, self.n_agents, 2)
        out = []
        for i in range(self.n_inst):
            rec = {k: float(m[i, j]) for j, k in enumerate(METRIC_KEYS)}
            rec["made_actions"], rec["init_positions"] = made[i], init[i].astype(int).tolist()
            out.append({"metrics": rec, "env_grid_search": dict(run_keys[i]), "algorithm": algorithm})
        return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="Run the expert over an evaluation config and write DIR/PIBT.json (or DIR/LaCAM.json)")
    ap.add_argument("--config", required=True, help="evaluation YAML (its environment: block is run)")
    ap.add_argument("--maps", default=None, help="maps.yaml ({name: map string}) registered on top of the built-in maps")
    ap.add_argument("--out", required=True, help="output directory")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--algo", choices=["pibt", "lacam"], default="pibt", help="lacam: a LaCAM search in front of every episode")
    ap.add_argument("--max-iters", type=int, default=4096, help="--algo lacam: iterations of the search per instance")
    ap.add_argument("--swap", action="store_true", help="the corridor swap rule in the generator (episode and search)")
    ap.add_argument("--refine-rounds", type=int, default=0, help="--algo lacam: rounds of the refinement pass over found solutions (0 = off)")
    ap.add_argument("--refine-horizon", type=int, default=None, help="solutions of up to this many steps are refined (default: twice the step cap)")
    a = ap.parse_args(argv)
    from . import evaluation as ev
    cfg = ev.load_yaml(a.config)
    reg = ev.MapRegistry()
    if a.maps:
        reg.register_maps(ev.load_yaml(a.maps))
    algo = {"name": "PIBT", "seed": a.seed, "device": a.device}
    if a.algo == "lacam":
        algo = {"name": "LaCAM", "seed": a.seed, "device": a.device, "max_iters": a.max_iters}
    if a.swap:
        algo["swap"] = True
    if a.refine_rounds:
        if a.algo != "lacam":
            ap.error("--refine-rounds needs --algo lacam")
        algo.update(refine_rounds=a.refine_rounds, refine_horizon=a.refine_horizon)
    cfg = {"environment": cfg["environment"], "algorithms": {algo["name"]: algo}}
    status, refine = {}, {}
    t0 = time.perf_counter()
    res = ev.evaluation(cfg, eval_dir=a.out, registry=reg, print_fn=lambda *_: None, log_actions=True, search_status=status,
                        refine_stats=refine)
    solved = [r for r in res if r["metrics"]["CSR"] >= 1]
    rows = sum(len(r["metrics"]["made_actions"]) * (int(r["metrics"]["ep_length"]) + 1) for r in solved)     # dataset rows of the solved episodes
    line = {"episodes": len(res), "solved": len(solved), "rows": rows, "seconds": round(time.perf_counter() - t0, 3)}
    if a.algo == "lacam":
        line["status"] = {str(k): int(v) for k, v in sorted(status.items())}
    if a.swap:
        line["swap"] = True
    if a.refine_rounds:
        line.update(refine_rounds=a.refine_rounds, **{k: int(refine.get(k, 0)) for k in ("refined", "rescued", "soc_before", "soc_after")})
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
