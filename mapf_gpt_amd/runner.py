"""Device-resident episode loop: env step -> tokenizer -> policy -> actions for many instances, with
instance sharding across the GPUs of a node and ONE collective (metrics all_gather) at the end.

This is what replaces the reference's episode-level process pool (dask workers each running
run_episode with its own model copy: eval_configs/01-random/01-random.yaml:147-148, inference.py:30-31,
121-125): instances are batched on one GPU and partitioned over ranks; no per-step traffic leaves
the GPU and nothing synchronises with the host inside the loop.

One hot-path step (order as in the reference's run_episode loop, example.py:65 / inference.py:142-168):
    tokenizer.update_agents(env.pos, env.goal, last_actions)   # history gets the previous INTENDED actions
    tokens  = tokenizer.generate_observations()                # uint8 [rows, 256]
    actions = policy.act(tokens)                               # int32 [rows]
    env.step(actions); last_actions = actions

retire_done=True (opt-in) stops forwarding finished instances: every poll_every-th step the library compacts the ids of the
instances that are not done and reads their count back (the mode's only host synchronisation); until the next poll the policy
runs on the token rows of those instances alone.  Draws and metrics are those of the plain run ("Retire mode").

shield="pibt" (opt-in) puts a collision shield between the policy and the env: every step the sampled actions
and the logits go through one PIBT step per instance, with each agent's candidates in the policy's order of preference, and the env
executes the planned actions -- nobody steps into a conflict, so the env's rules never make an agent wait.

shield_lifelong=True (opt-in, with shield="pibt") runs that shield on lifelong episodes: the runner is then
lifelong-only, reset() needs a goal_queue, the plan reads the fields of the goals the agents hold now (the step's own update_agents
rebuilds them) and arrivals() is the count of arrivals per instance and step.  Without it a shield refuses a goal_queue as before.

record=True (opt-in) keeps the episode on the device: one more launch per step stores every agent's position after
the step and the action the env was handed; trajectory() hands the buffers out as tensors, records() as toolbox records with
`made_actions`, `init_positions` and `moves` (the action the env executed), which is what mapf_gpt_amd.ddg relabels.
"""
import ctypes

import numpy as np
import torch

from . import _lib, maps
from .env import BatchedEnv
from .observation_generator import BatchedTokenizer


def shard_range(n_total, rank, world):
    """Contiguous instance range [lo, hi) of `rank` (sizes differ by at most one)."""
    base, rem = divmod(n_total, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def gather_metrics(local, n_total, rank=0, world=1, group=None, force=False):
    """all_gather of per-instance metric records float32 [n_local, 5] -> [n_total, 5] on every rank.
    The only collective of the job (RCCL over xGMI with backend "nccl"; gloo on CPU for tests);
    ~20 B x instances, latency-bound -- one call, no ring tuning.  force: take the collective at world = 1 too (a process
    group of one rank: how the RCCL branch is exercised on a one-GPU box, tests/test_gpu_bench.py)."""
    if world == 1 and not force:
        return local
    import torch.distributed as dist
    dev = local.device
    if local.is_cuda and dist.get_backend(group) == "gloo":      # CPU collectives (tests, dry runs): stage through the host
        local = local.cpu()
    counts = [shard_range(n_total, r, world)[1] - shard_range(n_total, r, world)[0] for r in range(world)]
    pad = max(counts)
    buf = torch.zeros((pad, local.shape[1]), dtype=local.dtype, device=local.device)
    buf[: local.shape[0]] = local
    out = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(out, buf, group=group)
    return torch.cat([o[:c] for o, c in zip(out, counts)], dim=0).to(dev)


def make_instances(grid, n_inst, n_agents, first_seed=0, start_ok=None, goal_ok=None):
    """Seeded starts/goals for instances first_seed .. first_seed+n_inst-1 on one shared padded map
    (instance i uses seed i: SURVEY.md section 8d) -> int16 tensors [n_inst, n_agents, 2]."""
    comp = maps.largest_component(grid == 0)
    pos = np.empty((n_inst, n_agents, 2), dtype=np.int16)
    goal = np.empty((n_inst, n_agents, 2), dtype=np.int16)
    for i in range(n_inst):
        pos[i], goal[i] = maps.place_agents(grid, n_agents, first_seed + i, start_ok, goal_ok, component=comp)
    return torch.from_numpy(pos), torch.from_numpy(goal)


def moves_from_positions(pos):
    """pos integer tensor [T + 1, ..., 2] -> int8 [T, ...]: the action the env executed between consecutive slots, the unique k with
    pos[t] + move[k] == pos[t + 1] (0 wait, 1 up, 2 down, 3 left, 4 right; 0 where the env made the agent wait)."""
    d = pos[1:].to(torch.int32) - pos[:-1].to(torch.int32)
    dr, dc = d[..., 0], d[..., 1]
    k = torch.zeros_like(dr)
    for code, (r, c) in ((1, (-1, 0)), (2, (1, 0)), (3, (0, -1)), (4, (0, 1))):
        k = torch.where((dr == r) & (dc == c), torch.full_like(k, code), k)
    return k.to(torch.int8)


class BatchedRunner:
    shield_lifelong = False

    def __init__(self, grids, n_inst, n_agents, net, max_episode_steps=128, seed=0, do_sample=True, precision=None,
                 device="cuda", row_offset=0, use_graph=False, retire_done=False, poll_every=8, shield=None, record=False,
                 shield_lifelong=False):
        if shield not in (None, "pibt"):
            raise ValueError(f"shield={shield!r}: None or 'pibt'")
        if shield_lifelong and shield != "pibt":
            raise ValueError("shield_lifelong=True needs shield='pibt': it is the shield that runs on lifelong episodes")
        if retire_done and use_graph:
            raise ValueError("retire_done=True runs eager launches only: the policy's row count changes from poll to poll, use_graph=True cannot replay it")
        if int(poll_every) < 1:
            raise ValueError("poll_every must be >= 1")
        self.device = torch.device(device)
        self.env = BatchedEnv(grids, n_inst, n_agents, max_episode_steps, device=device)
        self.tok = BatchedTokenizer(grids, n_inst, n_agents, device=device)
        self.net = net
        self.n_inst, self.n_agents = n_inst, n_agents
        self.rows = n_inst * n_agents
        self.seed, self.do_sample, self.precision = seed, do_sample, precision
        self.row_offset = row_offset          # global row id of this shard's first row: the sampler keys draws by global row
        self.tokens = torch.empty((self.rows, 256), dtype=torch.uint8, device=self.device)
        self.actions = torch.full((n_inst, n_agents), -1, dtype=torch.int32, device=self.device)
        self.t = 0
        self._pos_ptr, self._goal_ptr, _ = self.env.state_ptrs()
        # the whole step behind one library call.  use_graph=True replays it as a hipGraph after the first (eager) step: an OPTION since
        # round 5, not the default -- a cfg1 step is 19 dependent launches that keep the GPU 97 % busy, so the replay has no launch cost
        # to remove (0.279 ms against 0.272 ms eager, BENCH_r04); it stays for callers that want the host out of the loop, and
        # tests/test_gpu_step_graph.py keeps it bit-identical to the eager path
        self.use_graph = bool(use_graph)
        self._step = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mgpt_step_create(ctypes.byref(self._step), self.tok._h, self.net._h, self.env._h, self.rows,
                                                   _lib.PRECISIONS[precision or net.precision], 1 if do_sample else 0,
                                                   int(seed) & (2 ** 64 - 1), int(row_offset)))
        # retire mode: live_instances = count at the last poll, rows_forwarded = rows sent through the policy since reset()
        self.retire_done, self.poll_every = False, int(poll_every)
        self._live, self._rows_forwarded, self._polled_t = n_inst, 0, -1
        if retire_done:
            self.set_retire_done(True)
        self.shield, self._shield, self.shield_lifelong = shield, None, bool(shield_lifelong)
        if shield:
            from .expert import BatchedExpert
            # (shield_lifelong: switched here, once, before the env gets its queues in reset())
            self._shield = BatchedExpert(grids, n_inst, n_agents, max_episode_steps, device=device, shield=True, env=self.env, tok=self.tok,
                                         **({"shield_lifelong": True} if shield_lifelong else {}))
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().mgpt_step_set_shield(self._step, self._shield._h))
        self.record = False
        if record:
            self.set_record(True)

    def set_record(self, on):
        """Switch the episode recorder (mgpt_step_set_record: allocates / frees its buffers); a recording starts at the next reset()."""
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mgpt_step_set_record(self._step, 1 if on else 0))
        self.record = bool(on)

    def trajectory(self):
        """record=True: (pos int16 [T + 1, n_inst, n_agents, 2], actions int8 [T, n_inst, n_agents], lengths int32 [n_inst]) device
        tensors, T = max_episode_steps.  Slot 0 of pos is the reset positions, slot t + 1 the positions after step t; actions[t] is
        what the env was handed at step t (with a shield: the planned action).  Instance i is valid up to lengths[i], the env's
        ep_length: pos[lengths[i]] is where it ended (and every later slot that was stepped repeats it), actions beyond are meaningless."""
        T = self.env.max_episode_steps
        pos = torch.empty((T + 1, self.n_inst, self.n_agents, 2), dtype=torch.int16, device=self.device)
        act = torch.empty((T, self.n_inst, self.n_agents), dtype=torch.int8, device=self.device)
        with _lib.on_device(self.device):
            _lib.check(_lib.lib().mgpt_step_copy_record(self._step, _lib.ptr(pos), _lib.ptr(act), _lib.stream_ptr()))
        return pos, act, self.metrics()[:, 4].to(torch.int32)

    def records(self, run_keys, algorithm="MAPF-GPT"):
        """record=True: toolbox result records in BatchedExpert.records' shape -- the six env metrics, `init_positions` (slot 0, padded
        coordinates), `made_actions` (per agent, the actions the env was handed, cut to the episode's length) and `moves`: the action
        the env executed, from the recorded positions.  dataset_tokenizer.agent_paths(init_positions, moves) is the recorded path;
        with made_actions it is not wherever the env turned a move into a wait."""
        pos, act, lens = self.trajectory()
        moves = moves_from_positions(pos).permute(1, 2, 0).cpu().numpy()
        made = act.permute(1, 2, 0).cpu().numpy()
        init, lens, m = pos[0].cpu().numpy(), lens.cpu().numpy(), self.metrics().cpu().numpy()
        from .env import METRIC_KEYS
        out = []
        for i in range(self.n_inst):
            rec = {k: float(m[i, j]) for j, k in enumerate(METRIC_KEYS)}
            n = int(lens[i])
            rec["made_actions"] = [made[i, a, :n].tolist() for a in range(self.n_agents)]
            rec["moves"] = [moves[i, a, :n].tolist() for a in range(self.n_agents)]
            rec["init_positions"] = init[i].astype(int).tolist()
            out.append({"metrics": rec, "env_grid_search": dict(run_keys[i]), "algorithm": algorithm})
        return out

    def shield_overrides(self):
        """int32 [n_inst]: agents whose planned action was not the sampled one, summed over the steps since reset() (device tensor)."""
        if self._shield is None:
            raise RuntimeError("shield_overrides() needs shield='pibt'")
        return self._shield.shield_overrides()

    def arrivals(self):
        """shield_lifelong=True: int16 [n_inst, T] arrivals per instance and step since reset() (device tensor; T = max_episode_steps);
        an instance's sum is the env's own arrival count, the figure behind avg_throughput."""
        if not self.shield_lifelong:
            raise RuntimeError("arrivals() needs shield='pibt' with shield_lifelong=True")
        return self._shield.arrivals()

    def shield_state(self):
        """Tests: (logits float32 [rows, 67], first int32 [n_inst, n_agents], actions int32 [n_inst, n_agents], planned int16 [n_inst,
        n_agents, 2]) of the last step.  In retire mode the logits are the compact rows of live_state()."""
        if self._shield is None:
            raise RuntimeError("shield_state() needs shield='pibt'")
        if self.retire_done:
            logits = self.live_state()[1]
        else:
            logits = torch.empty((self.rows, 67), dtype=torch.float32, device=self.device)
            with _lib.on_device(self.device):
                _lib.check(_lib.lib().mgpt_step_copy_shield_logits(self._step, _lib.ptr(logits), _lib.stream_ptr()))
        return logits, self._shield.shield_first(), self.actions.clone(), self._shield.planned()

    def set_retire_done(self, on):
        """Switch retire mode (mgpt_step_set_retire: allocates / frees its buffers); takes effect at the next reset()."""
        if on and self.use_graph:
            raise ValueError("retire_done=True runs eager launches only, this runner replays a hipGraph (use_graph=True)")
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mgpt_step_set_retire(self._step, 1 if on else 0))
        self.retire_done = bool(on)

    @property
    def live_instances(self):
        return self._live

    @property
    def rows_forwarded(self):
        return self._rows_forwarded

    def __del__(self):
        h = getattr(self, "_step", None)
        if h:
            try:                   # (the step goes before the shield expert it points to)
                _lib.lib().mgpt_step_destroy(h)
            except Exception:      # interpreter shutdown
                pass
            self._step = None

    def reset(self, pos, goal, goal_queue=None):
        """goal_queue int16 [n_inst, n_agents, Q, 2]: lifelong mode (on_target="restart"), the tokenizer then re-checks
        goals every step (observation_generator.cpp:464-477)."""
        if self.shield_lifelong:
            if goal_queue is None:
                raise ValueError("shield_lifelong=True: reset() needs goal_queue, int16 [n_inst, n_agents, Q, 2] (the runner is lifelong-only)")
        elif goal_queue is not None and self._shield is not None:
            raise NotImplementedError("shield='pibt' does not plan lifelong (goal_queue) episodes")
        if goal_queue is not None or self.env.lifelong:
            self.env.set_lifelong(goal_queue)
        self.env.reset(pos, goal)
        self.tok.create_agents(self.env.pos, self.env.goal)
        self.actions.fill_(-1)                                   # inference.py:140
        self.t = 0
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mgpt_step_reset(self._step, 0, _lib.stream_ptr()))
        self._live, self._rows_forwarded, self._polled_t = self.n_inst, 0, -1
        if self._shield is not None:
            self._shield.reset_shield()
        if self.retire_done:
            self._poll()

    def _poll(self):
        """Rebuild the live list from the env's done flags and read its count back (synchronises the stream)."""
        n = ctypes.c_int(0)
        with _lib.on_device(self.device):
            _lib.check(_lib.lib().mgpt_step_poll_live(self._step, ctypes.byref(n), _lib.stream_ptr()))
        self._live, self._polled_t = int(n.value), self.t

    def _poll_if_due(self):
        if self.retire_done and self.t % self.poll_every == 0 and self._polled_t != self.t:
            self._poll()

    def live_state(self):
        """Retire mode, tests: (ids int32 [live_instances] of the live list, logits float32 [live_instances * n_agents, 67] of the
        last step's compact policy call)."""
        ids = torch.empty((self.n_inst,), dtype=torch.int32, device=self.device)
        logits = torch.empty((self.rows, 67), dtype=torch.float32, device=self.device)
        with _lib.on_device(self.device):
            _lib.check(_lib.lib().mgpt_step_copy_live(self._step, _lib.ptr(ids), _lib.ptr(logits), _lib.stream_ptr()))
        return ids[:self._live], logits[:self._live * self.n_agents]

    def step(self):
        """update_agents -> generate_observations -> act -> env.step in ONE library call (mgpt_step_run)."""
        self._poll_if_due()
        with _lib.on_device(self.device):
            _lib.check(_lib.lib().mgpt_step_run(self._step, _lib.ptr(self.tokens), _lib.ptr(self.actions.view(-1)),
                                                1 if self.env.lifelong else 0, 1 if self.use_graph else 0, _lib.stream_ptr()))
        self._rows_forwarded += self._live * self.n_agents
        self.t += 1

    def run(self, steps):
        """`steps` steps; with retire_done it returns early once a poll reports no live instance (self.t = steps actually run)."""
        for _ in range(steps):
            if self.retire_done:
                self._poll_if_due()
                if self._live == 0:
                    return
            self.step()

    def metrics(self):
        return self.env.metrics()
