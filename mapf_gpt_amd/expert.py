"""Device-resident PIBT expert: the role of the reference's `run_expert()` (dataset/generate_dataset.py:214-230) with its logging
environment (experiment_setup/create_env.py:8-33, 49-60) -- step 1 of the dataset pipeline, and a baseline for the evaluation tables.

The reference's expert is LaCAM3 under POGEMA; neither is in its tree.  What runs here is PIBT (priority inheritance with
backtracking), the configuration generator of such a search, by this project's own spec, one wave64 workgroup per
instance on the BFS distance fields the tokenizer keeps in HBM.  It is a WEAKER teacher than LaCAM: nothing guarantees that all agents
stand on their goals at once, and episodes that do not end with CSR = 1 are dropped by the dataset tokenizer as the reference drops them.

    ex = BatchedExpert(grids, n_inst, n_agents, max_episode_steps, seed=0)
    ex.reset(pos, goal); ex.run(max_episode_steps)
    records = ex.records(run_keys, pos)            # toolbox records with made_actions / init_positions
    for ids, rows, labels in ex.dataset_rows(pos): # or straight to training rows on the device, grouped by grid

    python -m mapf_gpt_amd.expert --config CONFIG.yaml --maps MAPS.yaml --out DIR      # writes DIR/PIBT.json
    python -m mapf_gpt_amd.expert --algo lacam [--max-iters N] ...                      # writes DIR/LaCAM.json
    python -m mapf_gpt_amd.expert [--algo lacam] --swap ...                             # the same files, with the corridor swap rule
    python -m mapf_gpt_amd.expert --algo lacam --refine-rounds N [--refine-horizon H]   # ... with found solutions refined
    python -m mapf_gpt_amd.expert --lifelong [--swap] ...                               # on_target: restart configs, DIR/PIBT.json
    python -m mapf_gpt_amd.expert ... --shards PREFIX --desired-size N                  # .arrow shards straight from the device log
    python -m mapf_gpt_amd.expert ... --lifelong-shards PREFIX --desired-size N         # the same for on_target: restart configs

`search="lacam"` puts a LaCAM search (plain depth-first LaCAM over this PIBT as its configuration generator) in
front of the episode: reset() solves every instance on the device, an instance solved within the step cap replays its solution, every
other instance is planned step by step by PIBT as before, so the expert is never worse than PIBT alone.

`swap=True` turns on the corridor swap rule in the generator, both in the episode's plan kernel and inside the
search: two agents that meet head-on in a corridor walk together to the nearest junction and exchange there.  Off by default; with it
off every result is bit for bit what it was.

`refine_rounds=N` (search mode only) refines every found solution of up to `refine_horizon` steps before the episode (DESIGN.md section
26): rounds in which every agent is replanned once, alone, against the others' fixed paths, until a round changes nothing or N rounds
have run.  No agent's arrival ever grows, so a solution longer than the step cap may come under it and is then replayed.  Off by default.

`lifelong=True` plans lifelong episodes (on_target = restart): reset() takes the goal queues of the env
(`goal_queue` int16 [n_inst, n_agents, Q, 2], as BatchedRunner.reset), an agent that ends a step on the goal it pursued takes the next one
of its queue (the queue wraps) and its distance field is rebuilt inside the same step; episodes end by truncation only.  arrivals() is the
count of arrivals per instance and step, targets() every agent's list of goals as the dataset tokenizer walks it, and records() carries
it as `global_lifelong_targets_xy` with `avg_throughput` in the place of CSR .. makespan.  Not together with search=.  Off by default.

`shield=True` makes the context a collision shield for a policy instead of an expert of its own: PIBT with the
policy's action preferences as every agent's candidate order.  `env=` / `tok=` then name the BatchedEnv / BatchedTokenizer it plans on
(BatchedRunner(shield="pibt") passes its own); shield_step(logits, first) is plan -> env step -> since update, shield_overrides() the
count of agents per instance whose planned action was not the policy's.  step() and run() are refused.  Not together with search=,
swap=, refine_rounds= or lifelong=.  Off by default.

`shield_lifelong=True` (with shield=True) runs the shield on lifelong episodes: reset() takes the env's goal queues
as with lifelong=True, the plan is section 31's on the fields of the goals the agents hold now, and what follows the env step is section
30's: since against the goal held during the step, the arrivals of every step (arrivals(), throughput()).  shield_step() is then plan ->
env step -> tokenizer update (goals_may_change=1: the fields of the agents whose goal changed) -> commit.  Off by default.

The config is an evaluation YAML (eval_configs/<folder>/<folder>.yaml): its `environment:` block is run; its `algorithms:` block is
replaced by one PIBT entry (seed from --seed).  DIR/PIBT.json is what `dataset_build.split_by_map` and `dataset_build --logs` take
where the reference has LaCAM.json.  Prints one JSON line: episodes, solved, rows, seconds (with --algo lacam also `status`: the
count of instances per search status; with --swap also `"swap": true`; with --refine-rounds also `refine_rounds`, `refined`: instances
whose length or sum of costs fell, `rescued`: instances the search left over the step cap that are now replayed, and `soc_before` /
`soc_after`: the sum of costs summed over the refined instances).  With --lifelong (the config's environment must say `on_target:
restart`; not with --algo lacam) the line has `"lifelong": true`, `arrivals` (of all episodes) and `throughput` (arrivals per step, summed
over the agents, averaged over the episodes) in the place of `solved` -- a lifelong episode has no CSR -- and `rows` counts every episode.

`--shards PREFIX --desired-size N [--maze-ratio --files-per-chunk --num-chunks --shard-seed]` builds the training shards from the device
log as the episodes are planned (dataset_build.EpisodeStore / build_shards_from_store): the files that --out +
split_by_map + `dataset_build --logs` write, with no JSON in between.  --out is optional then (with both, the JSON is written too); the
line gains `chunks`, the chunk reports.  Not with --lifelong: that is `--lifelong-shards PREFIX --desired-size N [the same options]`
(DESIGN.md section 34), which implies --lifelong (same checks: on_target: restart, not with --algo lacam; not together with --shards)
and builds the shards of the lifelong episodes the same way -- every episode kept, the goal pursued at every timestep derived on the
device from the goal at reset, the queue and the arrival counts (BatchedExpert.lifelong_targets() -> EpisodeStore(lifelong=True)); `rows`
and `arrivals` are then counted on the device.  BatchedExpert.lifelong_rows(pos) is dataset_rows() for a lifelong expert.
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
    shield = shield_lifelong = False                              # (what reset()'s own checks read on an object that was never initialised)

    def __init__(self, grids, n_inst, n_agents, max_episode_steps, seed=0, device="cuda", inst_offset=0, search=None, max_iters=4096,
                 iters_per_launch=None, hash_bits=0, swap=False, refine_rounds=0, refine_horizon=None, lifelong=False, shield=False, env=None,
                 tok=None, shield_lifelong=False):
        if search not in (None, "lacam"):
            raise ValueError(f"search={search!r}: None or 'lacam'")
        if lifelong and search:
            raise ValueError("lifelong=True with search=: the search looks for a joint goal configuration, which a lifelong episode does not have")
        if refine_rounds and not search:
            raise ValueError("refine_rounds needs search='lacam': the pass refines what the search found")
        if shield and (search or swap or refine_rounds or lifelong):
            raise ValueError("shield=True with search=, swap=, refine_rounds= or lifelong=: the shield runs plain PIBT on the policy's candidate order")
        if shield_lifelong and not shield:
            raise ValueError("shield_lifelong=True needs shield=True: it switches what follows the env step of a shield-mode context")
        if (env is not None or tok is not None) and not shield:
            raise ValueError("env= / tok= need shield=True: an expert of its own makes its env and tokenizer")
        self.device = torch.device(device)
        self.env = env if env is not None else BatchedEnv(grids, n_inst, n_agents, max_episode_steps, device=device)
        self.tok = tok if tok is not None else BatchedTokenizer(grids, n_inst, n_agents, device=device)
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
        self.lifelong = False
        self._goal0 = self._queue = self._targets = None
        if lifelong:
            self.set_lifelong(True)
        self.shield = False
        self.shield_lifelong = False
        if shield:
            self.set_shield(True)
        if shield_lifelong:
            self.set_shield_lifelong(True)

    def set_shield_lifelong(self, on):
        """Turn the shield's lifelong mode on or off (shield mode only): before reset() or between episodes (MGPTError with ERR_STATE on a
        context that is not in shield mode, or in the middle of an episode); reset() must follow."""
        with _lib.on_device(self.device):
            _lib.check(_lib.lib().mgpt_expert_set_shield_lifelong(self._h, 1 if on else 0))
        self.shield_lifelong = bool(on)

    def set_shield(self, on):
        """Turn shield mode on or off: before reset() or between episodes (MGPTError with ERR_STATE in the middle of one, with
        ERR_UNSUPPORTED together with the search, the swap rule or lifelong planning); reset() must follow."""
        with _lib.on_device(self.device):
            _lib.check(_lib.lib().mgpt_expert_set_shield(self._h, 1 if on else 0))
        self.shield = bool(on)
        if not on:
            self.shield_lifelong = False                          # (the library releases section 35's buffers with the shield)

    def reset_shield(self):
        """Shield mode over a borrowed env and tokenizer (BatchedRunner): the expert's own part of reset(), after theirs."""
        self.actions.zero_()
        self.t = 0
        with _lib.on_device(self.device):
            _lib.check(_lib.lib().mgpt_expert_reset(self._h, _lib.stream_ptr()))

    def shield_step(self, logits, first):
        """logits float32 [n_inst * n_agents, >= 5] (or [n_inst, n_agents, >= 5]), first int32 [n_inst, n_agents]: the policy's logits and
        sampled actions -> the planned actions int32 [n_inst, n_agents] (self.actions), already executed by the env.  With
        shield_lifelong=True the tokenizer rebuilds the fields of the agents whose goal changed between the env step and the commit."""
        logits = logits.to(self.device, torch.float32).reshape(self.n_inst * self.n_agents, -1).contiguous()
        self.actions.copy_(first.to(self.device, torch.int32).reshape(self.n_inst, self.n_agents))
        with _lib.on_device(self.device):
            L, s = _lib.lib(), _lib.stream_ptr()
            _lib.check(L.mgpt_expert_shield(self._h, _lib.ptr(logits), int(logits.shape[1]), None, None, _lib.ptr(self.actions.view(-1)), s))
            _lib.check(L.mgpt_env_step(self.env._h, _lib.ptr(self.actions.view(-1)), s))
            if self.shield_lifelong:
                pos, goal, _ = self.env.state_ptrs()
                _lib.check(L.mgpt_tokenizer_update_agents(self.tok._h, pos, goal, _lib.ptr(self.actions.view(-1)), 1, s))
            _lib.check(L.mgpt_expert_shield_commit(self._h, s))
        self.t += 1
        return self.actions

    def shield_first(self):
        """int32 [n_inst, n_agents]: the policy's actions of the last shield step, as the planner read them (device tensor)."""
        out = torch.empty((self.n_inst, self.n_agents), dtype=torch.int32, device=self.device)
        with _lib.on_device(self.device):
            _lib.check(_lib.lib().mgpt_expert_copy_shield(self._h, _lib.ptr(out), None, _lib.stream_ptr()))
        return out

    def shield_overrides(self):
        """int32 [n_inst]: agents whose planned action was not the policy's, summed over the steps since reset() (device tensor)."""
        out = torch.empty((self.n_inst,), dtype=torch.int32, device=self.device)
        with _lib.on_device(self.device):
            _lib.check(_lib.lib().mgpt_expert_copy_shield(self._h, None, _lib.ptr(out), _lib.stream_ptr()))
        return out

    def set_lifelong(self, on):
        """Turn lifelong planning on or off: before reset() or between episodes (MGPTError with ERR_STATE in the middle of one, with
        ERR_UNSUPPORTED in search mode); reset() must follow."""
        with _lib.on_device(self.device):
            _lib.check(_lib.lib().mgpt_expert_set_lifelong(self._h, 1 if on else 0))
        self.lifelong = bool(on)

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

    def reset(self, pos, goal, goal_queue=None):
        """goal_queue int16 [n_inst, n_agents, Q, 2]: required with lifelong=True or shield_lifelong=True (the env's goal queues), refused
        without them."""
        if self.lifelong or self.shield_lifelong:
            if goal_queue is None:
                raise ValueError(f"{'lifelong' if self.lifelong else 'shield_lifelong'}=True: reset() needs goal_queue, int16 [n_inst, n_agents, Q, 2]")
            q = torch.as_tensor(goal_queue)
            if q.dim() != 4 or tuple(q.shape[:2]) != (self.n_inst, self.n_agents) or q.shape[2] < 1 or q.shape[3] != 2:
                raise ValueError(f"goal_queue {tuple(q.shape)}: [n_inst={self.n_inst}, n_agents={self.n_agents}, Q >= 1, 2]")
            self.env.set_lifelong(q)
            self._queue = q.cpu().numpy().astype(np.int64)
            self._goal0 = torch.as_tensor(goal).cpu().numpy().astype(np.int64).reshape(self.n_inst, self.n_agents, 2)
            # the same two on the device, goal first: every agent's target list as lifelong_targets() hands it on
            self._targets = torch.cat([torch.as_tensor(goal).to(self.device, torch.int16).reshape(self.n_inst, self.n_agents, 1, 2),
                                       q.to(self.device, torch.int16)], dim=2).contiguous()
        else:
            if goal_queue is not None:
                raise ValueError("goal_queue needs lifelong=True" + (" (a shield: shield_lifelong=True)" if self.shield else ""))
            if self.env.lifelong:                                 # an earlier lifelong episode on this context
                self.env.set_lifelong(None)
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

    def arrivals(self):
        """int16 [n_inst, T]: arrivals per instance and step (lifelong mode, or a shield with shield_lifelong=True; device tensor; T =
        max_episode_steps)."""
        out = torch.empty((self.n_inst, self.max_episode_steps), dtype=torch.int16, device=self.device)
        with _lib.on_device(self.device):
            _lib.check(_lib.lib().mgpt_expert_copy_arrivals(self._h, _lib.ptr(out), _lib.stream_ptr()))
        return out

    def targets(self):
        """Lifelong mode.  Per instance, per agent: [goal at reset] + [queue[k % Q] for k in range(arrivals of the agent)], cells as [r, c]
        in the env's (padded) coordinates -- the list dataset_tokenizer.goal_positions walks along the agent's path (host lists)."""
        if not self.lifelong or self._queue is None:
            raise RuntimeError("targets() needs lifelong=True and a reset()")
        reached = self.env.goals_reached().cpu().numpy()
        Q = self._queue.shape[2]
        return [[[self._goal0[i, a].tolist()] + [self._queue[i, a, k % Q].tolist() for k in range(int(reached[i, a]))]
                 for a in range(self.n_agents)] for i in range(self.n_inst)]

    def lifelong_targets(self):
        """Lifelong mode: targets() as the batched tokenizer takes it, with no host loop -> (targets int16 [n_inst, n_agents, 1 + Q, 2]: the
        goal at reset, then the queue as it lies (entry 1 + (j - 1) % Q is target j >= 1); n_targets int32 [n_inst, n_agents] = 1 + the
        agent's arrivals), device tensors."""
        if not self.lifelong or self._targets is None:
            raise RuntimeError("lifelong_targets() needs lifelong=True and a reset()")
        return self._targets, (self.env.goals_reached() + 1).to(torch.int32)

    def lifelong_rows(self, init_pos, tables=None, mask_cost2go=False, offsets=False):
        """dataset_rows() for a lifelong expert: the episodes since reset() as training rows with the goal pursued
        at every timestep, from the device log and lifelong_targets() in one tokenize_episodes call per distinct grid -> [(instance_ids,
        rows uint8 [N, 256], labels int8 [N])] (offsets=True: + row0) as dataset_rows returns them, every episode kept (a lifelong record has
        no CSR and the reference keeps it) -- what records() -> ObservationGenerator.generate_observations_device gives.  Raises IndexError
        where that route does: an agent that stood on more targets than its list holds (one that starts on its own goal)."""
        if not self.lifelong:
            raise RuntimeError("lifelong_rows() needs lifelong=True: the episodes of a one-shot expert go through dataset_rows()")
        if self._targets is None:
            raise RuntimeError("lifelong_rows() needs a reset(): there is no episode and no goal queue yet")
        from .dataset_tokenizer import TableCache, tokenize_episodes
        tables = tables if tables is not None else TableCache(device=self.device)
        init = torch.as_tensor(init_pos).to(self.device, torch.int16).reshape(self.n_inst, self.n_agents, 2)
        log, lens = self.log()
        targets, n_targets = self.lifelong_targets()
        out = []
        for ids, grid in self._instances_by_grid():
            rows, labels, row0 = tokenize_episodes(tables.get(grid), init, log, lens, None, ids, mask_cost2go, targets=targets,
                                                   n_targets=n_targets)
            out.append((ids, rows, labels, row0) if offsets else (ids, rows, labels))
        return out

    def _instances_by_grid(self):
        """[(instance ids int64, grid)] per distinct grid in order of first appearance (instance i uses grid i % n_grids)."""
        grids = self.env.grids.cpu().numpy()
        flat = grids.reshape(len(grids), -1)
        _, first, inverse = np.unique(flat, axis=0, return_index=True, return_inverse=True)
        of_inst = inverse.reshape(-1)[np.arange(self.n_inst) % len(grids)]
        out = []
        for u in np.argsort(first):
            ids = np.flatnonzero(of_inst == u).astype(np.int64)
            if len(ids):                                                                   # (a grid no instance uses: n_grids > n_inst)
                out.append((ids, grids[first[u]]))
        return out

    def throughput(self):
        """float32 [n_inst]: arrivals per step, summed over the agents, over max_episode_steps (lifelong mode; device tensor).  The
        counts are divided on the host, one correctly rounded float32 division each: torch's division of a device tensor by a scalar
        multiplies by the reciprocal, which is one unit in the last place off for 31 / 40."""
        total = self.env.goals_reached().sum(1).cpu().numpy()
        return torch.from_numpy(total.astype(np.float32) / np.float32(self.max_episode_steps)).to(self.device)

    def made_actions(self):
        """Per instance, per agent: the list of actions made, cut to the instance's episode length (host lists)."""
        log, lens = self.log()
        log, lens = log.cpu().numpy(), lens.cpu().numpy()
        return [[log[i, a, :int(lens[i])].tolist() for a in range(self.n_agents)] for i in range(self.n_inst)]

    def dataset_rows(self, init_pos, keep="solved", tables=None, mask_cost2go=False, offsets=False):
        """The episodes since reset() as training rows, from the expert's own device log with no host loop over episodes:
        -> [(instance_ids, rows uint8 [N, 256], labels int8 [N])], one entry per distinct grid in order of first appearance
        (instance_ids: int64 array, every instance on that grid; rows and labels: device tensors, the kept instances' rows in id order --
        what records() -> ObservationGenerator.generate_observations_device gives for them).  init_pos: the positions handed to
        reset().  keep: "solved" = CSR >= 1 from the env's metrics, taken on the device (the reference's filter); None = all; or a
        bool / uint8 tensor [n_inst].  tables: a dataset_tokenizer.TableCache to share the maps' tables between calls.  offsets=True
        adds a fourth entry, row0 int64 [len(instance_ids) + 1] (device): instance_ids[k] owns rows [row0[k], row0[k + 1])."""
        if self.lifelong:
            raise NotImplementedError("dataset_rows() has no per-step goals: a lifelong expert's episodes go through lifelong_rows(), or "
                                      "records() and dataset_tokenizer.ObservationGenerator")
        from .dataset_tokenizer import TableCache, tokenize_episodes
        tables = tables if tables is not None else TableCache(device=self.device)
        if isinstance(keep, str):
            if keep != "solved":
                raise ValueError(f"keep={keep!r}: 'solved', None or a tensor [n_inst]")
            keep = self.metrics()[:, METRIC_KEYS.index("CSR")] >= 1
        init = torch.as_tensor(init_pos).to(self.device, torch.int16).reshape(self.n_inst, self.n_agents, 2)
        log, lens = self.log()
        out = []
        for ids, grid in self._instances_by_grid():
            rows, labels, row0 = tokenize_episodes(tables.get(grid), init, log, lens, keep, ids, mask_cost2go)
            out.append((ids, rows, labels, row0) if offsets else (ids, rows, labels))
        return out

    def records(self, run_keys, init_pos, algorithm="PIBT"):
        """Toolbox result records (evaluation.py): metrics = the six env metrics + made_actions + init_positions (padded coordinates,
        as dataset_tokenizer.agent_paths expects), env_grid_search = run_keys[i], algorithm.  In lifelong mode the metrics are
        avg_throughput and ep_length (no CSR: dataset_tokenizer keeps such records) and global_lifelong_targets_xy = targets(), in the
        coordinates of init_positions."""
        m = self.metrics().cpu().numpy()
        made = self.made_actions()
        if self.lifelong:
            thr, tg = self.throughput().cpu().numpy(), self.targets()
        init = np.asarray(init_pos.cpu() if torch.is_tensor(init_pos) else init_pos).reshape(self.n_inst, self.n_agents, 2)
        out = []
        for i in range(self.n_inst):
            rec = {k: float(m[i, j]) for j, k in enumerate(METRIC_KEYS)}
            if self.lifelong:
                rec = {"avg_throughput": float(thr[i]), "ep_length": rec["ep_length"], "global_lifelong_targets_xy": tg[i]}
            rec["made_actions"], rec["init_positions"] = made[i], init[i].astype(int).tolist()
            out.append({"metrics": rec, "env_grid_search": dict(run_keys[i]), "algorithm": algorithm})
        return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="Run the expert over an evaluation config and write DIR/PIBT.json (or DIR/LaCAM.json)")
    ap.add_argument("--config", required=True, help="evaluation YAML (its environment: block is run)")
    ap.add_argument("--maps", default=None, help="maps.yaml ({name: map string}) registered on top of the built-in maps")
    ap.add_argument("--out", default=None, help="output directory (optional with --shards)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--algo", choices=["pibt", "lacam"], default="pibt", help="lacam: a LaCAM search in front of every episode")
    ap.add_argument("--max-iters", type=int, default=4096, help="--algo lacam: iterations of the search per instance")
    ap.add_argument("--swap", action="store_true", help="the corridor swap rule in the generator (episode and search)")
    ap.add_argument("--refine-rounds", type=int, default=0, help="--algo lacam: rounds of the refinement pass over found solutions (0 = off)")
    ap.add_argument("--refine-horizon", type=int, default=None, help="solutions of up to this many steps are refined (default: twice the step cap)")
    ap.add_argument("--lifelong", action="store_true", help="plan lifelong episodes: the config's environment must say on_target: restart")
    ap.add_argument("--shards", default=None, metavar="PREFIX", help="write .arrow shards from the device log (dataset_build.build_shards_from_store)")
    ap.add_argument("--desired-size", type=int, default=None, help="--shards: rows per chunk")
    ap.add_argument("--maze-ratio", type=float, default=0.9)
    ap.add_argument("--files-per-chunk", type=int, default=10)
    ap.add_argument("--num-chunks", type=int, default=1)
    ap.add_argument("--shard-seed", type=int, default=0, help="--shards: seed of the shuffles (dataset_build --seed)")
    ap.add_argument("--lifelong-shards", default=None, metavar="PREFIX",
                    help="--shards for lifelong episodes (implies --lifelong): the goal pursued at every timestep is derived on the device")
    a = ap.parse_args(argv)
    if a.lifelong_shards is not None:
        if a.shards is not None:
            ap.error("--lifelong-shards and --shards are two kinds of episodes: one store keeps one of them")
        if a.desired_size is None:
            ap.error("--lifelong-shards needs --desired-size")
        if a.algo == "lacam":
            ap.error("--lifelong-shards plans with PIBT only: the search of --algo lacam looks for a joint goal configuration")
        a.lifelong = True
    if a.shards is None and a.lifelong_shards is None and a.out is None:
        ap.error("one of --out, --shards and --lifelong-shards is required")
    if a.shards is not None and a.desired_size is None:
        ap.error("--shards needs --desired-size")
    if a.shards is not None and a.lifelong:
        ap.error("--shards does not take --lifelong: per-step goals go through --lifelong-shards, or the JSON log (--out) and "
                 "dataset_build --logs")
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
    if a.lifelong:
        if a.algo == "lacam":
            ap.error("--lifelong plans with PIBT only: the search of --algo lacam looks for a joint goal configuration")
        if cfg["environment"].get("on_target") != "restart":
            ap.error("--lifelong needs on_target: restart in the config's environment: block")
        algo["lifelong"] = True
    cfg = {"environment": cfg["environment"], "algorithms": {algo["name"]: algo}}
    status, refine = {}, {}
    store = None
    shards = a.shards if a.shards is not None else a.lifelong_shards
    if shards is not None:
        from .dataset_build import EpisodeStore
        store = EpisodeStore(device=a.device, lifelong=a.lifelong_shards is not None)
    t0 = time.perf_counter()
    res = ev.evaluation(cfg, eval_dir=a.out, registry=reg, print_fn=lambda *_: None, log_actions=a.out is not None, search_status=status,
                        refine_stats=refine, on_expert_batch=store.append if store is not None else None)
    solved = res if a.lifelong else [r for r in res if r["metrics"]["CSR"] >= 1]
    if a.out is not None and a.lifelong_shards is None:
        rows = sum(len(r["metrics"]["made_actions"]) * (int(r["metrics"]["ep_length"]) + 1) for r in solved)     # dataset rows of the solved episodes
    else:                                            # --shards alone: no action list ever reaches the host; --lifelong-shards: counted on the device
        rows = store.solved_rows()[1]
    line = {"episodes": len(res), "solved": len(solved), "rows": rows, "seconds": round(time.perf_counter() - t0, 3)}
    if a.lifelong:                                   # no CSR in a lifelong record: every episode gives rows
        del line["solved"]
        line["lifelong"] = True
        if a.lifelong_shards is not None:            # the store's lists: no target list reaches the host without --out
            line["arrivals"] = sum(int((b["n_targets"] - 1).sum()) for b in store.batches)
        else:
            line["arrivals"] = sum(len(tg) - 1 for r in res for tg in r["metrics"]["global_lifelong_targets_xy"])
        line["throughput"] = round(float(np.mean([r["metrics"]["avg_throughput"] for r in res])), 4) if res else 0.0
    if a.algo == "lacam":
        line["status"] = {str(k): int(v) for k, v in sorted(status.items())}
    if a.swap:
        line["swap"] = True
    if a.refine_rounds:
        line.update(refine_rounds=a.refine_rounds, **{k: int(refine.get(k, 0)) for k in ("refined", "rescued", "soc_before", "soc_after")})
    if store is not None:
        import os
        from .dataset_build import build_shards_from_store
        if os.path.dirname(shards):
            os.makedirs(os.path.dirname(shards), exist_ok=True)
        line["chunks"] = build_shards_from_store(store, shards, a.desired_size, a.maze_ratio, a.files_per_chunk, a.num_chunks, a.shard_seed)
        line["seconds"] = round(time.perf_counter() - t0, 3)
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
