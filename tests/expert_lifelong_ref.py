"""Plain Python restatement of the expert's lifelong mode on top of tests/expert_ref.py (section 20: bfs, the
generator, the env's collision rules) and tests/expert_swap_ref.py (section 22's rule) -- TEST INFRASTRUCTURE ONLY, written from the spec
and the env spec of section 4, not from the kernels.

    ref = RefLifelongExpert(grids, n_inst, n_agents, max_episode_steps, seed, inst_offset, swap=False)
    ref.reset(pos, goal, queue)            # queue [inst, agent, Q, 2]
    actions, planned = ref.step()

What it adds to RefExpert: the lifelong env rule (an agent that ends a step on the goal it pursued during that step is counted and takes
the next goal of its own queue, which wraps; the episode ends by truncation only), the field of a new goal, the `since` rule on the goal
held DURING the step, the arrivals of every step, and goal_hist: the goals after reset and after every step.
"""
import numpy as np

from tests import expert_ref as er
from tests import expert_swap_ref as sw


class RefLifelongExpert(sw.RefSwapExpert):
    def __init__(self, grids, n_inst, n_agents, max_episode_steps, seed=0, inst_offset=0, swap=False):
        super().__init__(grids, n_inst, n_agents, max_episode_steps, seed, inst_offset, swap=swap)

    def reset(self, pos, goal, queue):
        super().reset(pos, goal)
        self.queue = np.asarray(queue, np.int64).reshape(self.n_inst, self.n_agents, -1, 2).copy()
        self.goal0 = self.goal.copy()
        self.qnext = np.zeros((self.n_inst, self.n_agents), np.int64)
        self.reached = np.zeros((self.n_inst, self.n_agents), np.int64)
        self.arrivals = [[] for _ in range(self.n_inst)]
        self.goal_hist = [self.goal.copy()]

    def step(self):
        n_inst, n, Q = self.n_inst, self.n_agents, self.queue.shape[2]
        actions = np.zeros((n_inst, n), np.int32)
        planned = self.pos.astype(np.int16).copy()                # a done instance plans to stay where it is
        for i in range(n_inst):
            if self.done[i]:
                continue
            grid = self.grid(i)
            nxt, act = self.plan_instance(i)                      # section 20's (22's) plan on pos, the current goals' fields and since
            actions[i], planned[i] = act, np.asarray(nxt, np.int16)
            for a in range(n):
                self.made[i][a].append(int(act[a]))
            self.pos[i] = np.asarray(er.env_step(grid, self.pos[i], act), np.int64)
            self.tcount[i] += 1
            on = (self.pos[i] == self.goal[i]).all(-1)            # against the goal pursued during this step
            for a in np.flatnonzero(on):
                self.reached[i, a] += 1
                self.goal[i, a] = self.queue[i, a, self.qnext[i, a]]
                self.qnext[i, a] = (self.qnext[i, a] + 1) % Q
                self.dist[i][a] = er.bfs(grid, self.goal[i, a])
            self.dens[i].append(er.density_sample(grid, self.pos[i]))
            self.since[i] = np.where(on, 0, self.since[i] + 1)
            self.arrivals[i].append(int(on.sum()))
            if self.tcount[i] >= self.max_steps:
                self.done[i] = 2
        self.t += 1
        self.goal_hist.append(self.goal.copy())
        return actions, planned

    def arrivals_log(self):
        """int16 [inst, max_steps], 0 beyond the steps made."""
        out = np.zeros((self.n_inst, self.max_steps), np.int16)
        for i, arr in enumerate(self.arrivals):
            out[i, :len(arr)] = arr
        return out

    def targets(self):
        """Per instance and agent: [goal at reset] + [queue[k % Q] for k in range(reached)]."""
        Q = self.queue.shape[2]
        return [[[self.goal0[i, a].tolist()] + [self.queue[i, a, k % Q].tolist() for k in range(int(self.reached[i, a]))]
                 for a in range(self.n_agents)] for i in range(self.n_inst)]

    def throughput(self):
        """float32 [inst]: arrivals per step, summed over the agents, over max_steps -- one correctly rounded float32 division, as BatchedExpert.throughput forms it."""
        return self.reached.sum(1).astype(np.float32) / np.float32(self.max_steps)


def records(ref, run_keys, init_pos, algorithm="PIBT"):
    """The record shape of BatchedExpert.records in lifelong mode, from the restatement's state."""
    thr, tg, ep = ref.throughput(), ref.targets(), ref.metrics()[:, 4]
    out = []
    for i in range(ref.n_inst):
        rec = {"avg_throughput": float(thr[i]), "ep_length": float(ep[i]), "global_lifelong_targets_xy": tg[i],
               "made_actions": [list(a) for a in ref.made[i]], "init_positions": np.asarray(init_pos[i]).astype(int).tolist()}
        out.append({"metrics": rec, "env_grid_search": dict(run_keys[i]), "algorithm": algorithm})
    return out


# ---- the shapes both test files use -------------------------------------------------------------------------------------------
_OPEN6 = ["......"] * 6


def _queue(per_agent):
    """[[cells of agent 0's queue], ...] (unpadded) -> int16 [1, agents, Q, 2] padded."""
    return np.asarray(per_agent, np.int16).reshape(1, len(per_agent), -1, 2) + er.PAD


def hand_cases():
    """name -> dict(grids, n_inst, n_agents, pos, goal, queue, steps, seed, inst_offset, swap).  Coordinates are padded."""
    c = {}
    # one agent on an open 6 x 6 and a queue of three: legs of 5, 6, 8, 4 steps, then 4 to queue[0] again (the wrap) and 8 to queue[1]: six arrivals in 35 steps
    c["wrap1"] = dict(grids=er._parse(_OPEN6), pos=er._cells([(0, 0)]), goal=er._cells([(2, 3)]), queue=_queue([[(5, 0), (1, 4), (5, 4)]]), steps=36)
    # the next queued goal is the cell the agent stands on when it arrives: its wait on the following step is a second arrival
    c["own_cell"] = dict(grids=er._parse(_OPEN6), pos=er._cells([(0, 0)]), goal=er._cells([(0, 2)]), queue=_queue([[(0, 2), (3, 2), (0, 2)]]), steps=12)
    # two consecutive queue entries are the same cell
    c["duplicates"] = dict(grids=er._parse(_OPEN6), pos=er._cells([(5, 5)]), goal=er._cells([(5, 3)]), queue=_queue([[(2, 3), (2, 3), (4, 0)]]), steps=16)
    # two agents bound for the same cell, again and again
    c["same_goal2"] = dict(grids=er._parse(_OPEN6), pos=er._cells([(0, 0), (5, 5)]), goal=er._cells([(2, 2), (2, 2)]),
                           queue=_queue([[(4, 1), (0, 5)], [(4, 1), (0, 5)]]), steps=24)
    # section 20's corridor with a side pocket: agent 0 arrives first, its since falls to 0 and agent 1 plans first from then on
    pocket = er.hand_cases()["pocket"]
    c["pocket"] = dict(grids=pocket["grids"], pos=pocket["pos"], goal=pocket["goal"],
                       queue=_queue([[(1, 1), (1, 3)], [(1, 3), (1, 1)]]), steps=16)
    for v in c.values():
        v.update(n_inst=1, n_agents=v["pos"].shape[1], seed=3, inst_offset=0, swap=False)
    return c


def _queues(grids, n_inst, n_agents, Q, inst_offset):
    """Seeded queues: cells of the largest free component of the instance's grid."""
    from mapf_gpt_amd import maps
    cells = [np.argwhere(maps.largest_component(g == 0)) for g in grids]
    queue = np.empty((n_inst, n_agents, Q, 2), np.int16)
    for i in range(n_inst):
        rng = np.random.Generator(np.random.PCG64([100 + inst_offset + i, 0x4C4C]))
        cl = cells[i % len(grids)]
        queue[i] = cl[rng.integers(0, len(cl), (n_agents, Q))]
    return queue


def _no_agent_starts_on_its_goal(case):
    """Standing on the goal at reset is no arrival for the env but advances dataset_tokenizer.goal_positions' list (DESIGN.md section
    30): the goals of an instance rotate by one agent until no agent starts on its own."""
    for i in range(case["n_inst"]):
        for _ in range(case["n_agents"]):
            if not (case["pos"][i] == case["goal"][i]).all(-1).any():
                break
            case["goal"][i] = np.roll(case["goal"][i], 1, axis=0)
        assert not (case["pos"][i] == case["goal"][i]).all(-1).any()
    return case


def random_case(h, w, density, n_inst, n_agents, steps, seed, Q=8, n_grids=1, inst_offset=0, swap=False):
    case = er.random_case(h, w, density, n_inst, n_agents, steps, seed, n_grids=n_grids, inst_offset=inst_offset)
    case.update(queue=_queues(case["grids"], n_inst, n_agents, Q, inst_offset), swap=swap)
    return _no_agent_starts_on_its_goal(case)


def maze_case(n_agents=8, n_inst=2, steps=48, seed=7, Q=8, swap=True):
    """The dataset's 21 x 21 maze (corridors: the swap rule's ground) with 8 agents."""
    case = sw.maze_case(n_agents, n_inst, steps, seed)
    case.update(queue=_queues(case["grids"], n_inst, n_agents, Q, 0), swap=swap)
    return _no_agent_starts_on_its_goal(case)


def gpu_cases():
    """The shapes of tests/test_gpu_expert_lifelong.py (and of the digests pinned in tests/test_expert_lifelong_cpu.py)."""
    c = hand_cases()
    c["one_agent"] = random_case(12, 12, 0.2, 1, 1, 40, seed=1, Q=2)       # more arrivals than queue entries
    c["agents65"] = random_case(16, 16, 0.2, 1, 65, 48, seed=5, Q=4)       # the first counts at which the strided loops stride past
    c["agents70"] = random_case(16, 16, 0.2, 1, 70, 48, seed=6, Q=4)       # one wave; the queues wrap
    c["grids3"] = random_case(12, 12, 0.2, 3, 8, 40, seed=7, n_grids=3)
    c["shared5"] = random_case(12, 12, 0.2, 5, 8, 40, seed=8)
    c["offset7"] = random_case(12, 12, 0.2, 3, 8, 40, seed=10, inst_offset=7)
    c["maze8_swap"] = maze_case()
    return c


def new_ref(case):
    ref = RefLifelongExpert(case["grids"], case["n_inst"], case["n_agents"], case["steps"], case["seed"], case["inst_offset"], case["swap"])
    ref.reset(case["pos"], case["goal"], case["queue"])
    return ref


def run_case(case, steps=None):
    ref = new_ref(case)
    ref.run(case["steps"] if steps is None else steps)
    return ref
