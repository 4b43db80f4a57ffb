"""Plain Python restatement of the corridor swap rule on top of tests/expert_ref.py (section 20) and
tests/expert_search_ref.py (section 21) -- TEST INFRASTRUCTURE ONLY, written from the spec, not from the kernels.

    nxt, act, depth = plan(grid, pos, dist, since, seed, t, row0, swap=True)
    out = gen(grid, Q, dist, since, order, chain, seed, t, row0, swap=True)
    out = search(grid, pos, goal, dist, seed, row0, max_iters, max_steps, swap=True)
    ref = RefSwapExpert(...); ref = RefSwapSearchExpert(...)          # RefExpert / RefSearchExpert with swap=True by default

Every function here is the one of those two files with Rule handed to the generator (swap=False: without it).  `cap` (test-only)
replaces the walk cap H * W.  `trace`, a dict, counts the branches a call went through, so that a test can tell that a hand case
reaches the branch it was drawn for.
"""
import functools

import numpy as np

from tests import expert_ref as er
from tests import expert_search_ref as sr


class Rule:
    """The swap rule on one state: grid, current cells `pos`, `occ_now`, the decisions `nxt` (None = undecided), `next_occ`."""

    def __init__(self, grid, pos, dist, occ_now, nxt, act, next_occ, cap=None, trace=None):
        self.grid, self.pos, self.dist, self.occ_now, self.nxt, self.act, self.next_occ = grid, pos, dist, occ_now, nxt, act, next_occ
        self.H, self.W = grid.shape
        self.cap = self.H * self.W if cap is None else cap
        self.trace = trace if trace is not None else {}

    def note(self, what):
        self.trace[what] = self.trace.get(what, 0) + 1

    def free(self, u):
        return 0 <= u[0] < self.H and 0 <= u[1] < self.W and self.grid[u] == 0

    def neighbours(self, v):
        """The free 4-neighbours of v in action order 1..4."""
        return [u for u in ((v[0] + dr, v[1] + dc) for dr, dc in er.MOVES[1:]) if self.free(u)]

    def deg(self, v):
        return len(self.neighbours(v))

    def D(self, a, v):
        return int(self.dist[a][v])

    def rests(self, u):
        b = self.occ_now.get(u)
        return self.deg(u) == 1 and b is not None and self.D(b, u) == 0

    def count(self, v_pusher, v_puller):
        n, other = self.deg(v_puller), None
        for u in self.neighbours(v_puller):
            if u == v_pusher:
                n -= 1
            elif self.rests(u):
                n -= 1
                self.note("rests")
            else:
                other = u
        return n, other

    def required(self, pusher, puller, v_pusher, v_puller):
        for _ in range(self.cap):
            if not self.D(pusher, v_puller) < self.D(pusher, v_pusher):
                break
            n, other = self.count(v_pusher, v_puller)
            if n >= 2:
                return False
            if n <= 0:
                break
            v_pusher, v_puller = v_puller, other
        else:
            self.note("cap")
        return self.D(puller, v_pusher) < self.D(puller, v_puller) and (
            self.D(pusher, v_pusher) == 0 or self.D(pusher, v_puller) < self.D(pusher, v_pusher))

    def possible(self, v_pusher, v_puller):
        origin = v_pusher
        for _ in range(self.cap):
            if v_puller == origin:
                self.note("ring")
                return False
            n, other = self.count(v_pusher, v_puller)
            if n >= 2:
                return True
            if n <= 0:
                return False
            v_pusher, v_puller = v_puller, other
        self.note("cap")
        return False

    def swap_agent(self, a, C):
        """C: a's sorted candidates (key, k, u).  -> the swap agent or None."""
        if not C or C[0][2] == self.pos[a]:
            return None
        pa, c0 = self.pos[a], C[0][2]
        j = self.occ_now.get(c0)
        if j is not None and self.nxt[j] is None and self.required(a, j, pa, self.pos[j]) and self.possible(self.pos[j], pa):
            self.note("swap")
            return j
        for u in self.neighbours(pa):
            b = self.occ_now.get(u)
            if b is None or u == c0:
                continue
            if self.required(b, a, pa, c0) and self.possible(c0, pa):
                self.note("clear")
                return b
        return None

    def order(self, a, C):
        """-> (candidates in the order they are tried, swap agent)."""
        j = self.swap_agent(a, C)
        return (C[::-1] if j is not None else C), j

    def pull(self, a, j, first):
        """On PIBT(a)'s success return; `first`: the candidate taken was the first of the list as tried."""
        if j is None:
            return
        pa = self.pos[a]
        if not first:
            return
        if self.nxt[j] is not None:
            self.note("pull_decided")
            return
        if pa in self.next_occ:
            self.note("pull_own" if self.nxt[a] == pa else "pull_reserved")
            return
        self.nxt[j] = pa
        self.act[j] = er.MOVES.index((pa[0] - self.pos[j][0], pa[1] - self.pos[j][1]))
        self.next_occ[pa] = j
        self.note("pull")


def _rule(swap, cap, trace):
    """The `rule` argument of expert_ref.gen: Rule on the generator's state, or None with the switch off."""
    return functools.partial(Rule, cap=cap, trace=trace) if swap else None


def plan(grid, pos, dist, since, seed, t, row0, swap=True, cap=None, trace=None):
    """expert_ref.plan with the rule: -> (next cells, actions, deepest stack reached)."""
    return er.gen(grid, pos, dist, since, er.priority_order(since), (), seed, t, row0, _rule(swap, cap, trace))


def gen(grid, Q, dist, since, order, chain, seed, t, row0, swap=True, cap=None, trace=None):
    """expert_search_ref.gen with the rule: -> (next cells, actions) or None on failure."""
    return sr.gen(grid, Q, dist, since, order, chain, seed, t, row0, _rule(swap, cap, trace))


def search(grid, pos, goal, dist, seed, row0, max_iters, max_steps, swap=True, cap=None, trace=None):
    """expert_search_ref.search over the generator with the rule (the search itself is section 21's, unchanged)."""
    return sr.search(grid, pos, goal, dist, seed, row0, max_iters, max_steps, _rule(swap, cap, trace))


class _Swap:
    """Both experts with the switch: `rule` is what plan_instance() and the search hand to the generator."""

    def set_swap(self, swap, cap):
        self.swap, self.cap, self.trace = bool(swap), cap, {}
        self.rule = _rule(self.swap, cap, self.trace)


class RefSwapExpert(_Swap, er.RefExpert):
    def __init__(self, grids, n_inst, n_agents, max_episode_steps, seed=0, inst_offset=0, swap=True, cap=None):
        super().__init__(grids, n_inst, n_agents, max_episode_steps, seed, inst_offset)
        self.set_swap(swap, cap)


class RefSwapSearchExpert(_Swap, sr.RefSearchExpert):
    def __init__(self, grids, n_inst, n_agents, max_episode_steps, seed=0, inst_offset=0, max_iters=4096, swap=True, cap=None):
        super().__init__(grids, n_inst, n_agents, max_episode_steps, seed, inst_offset, max_iters)
        self.set_swap(swap, cap)


def run_case(case, steps=None, swap=True, cap=None):
    ref = RefSwapExpert(case["grids"], case["n_inst"], case["n_agents"], case["steps"], case["seed"], case["inst_offset"], swap, cap)
    ref.reset(case["pos"], case["goal"])
    ref.run(case["steps"] if steps is None else steps)
    return ref


def run_search_case(case, steps=None, max_iters=None, swap=True, cap=None):
    ref = RefSwapSearchExpert(case["grids"], case["n_inst"], case["n_agents"], case["steps"], case["seed"], case["inst_offset"],
                              case.get("max_iters", 512) if max_iters is None else max_iters, swap, cap)
    ref.reset(case["pos"], case["goal"])
    ref.run(case["steps"] if steps is None else steps)
    return ref


# ---- the shapes both test files use -------------------------------------------------------------------------------------------
_RING = ["#####", "#...#", "#.#.#", "#...#", "#####"]
_RING_SPUR = ["#######", "#.....#", "#.###.#", "#.....#", "###.###", "#######"]
_STUB = ["######", "##.###", "#....#", "######"]

# hand case -> the branch (a key of `trace`) it was drawn for, and the step of the episode at which it is reached first
BRANCH = {"clear2": ("clear", 1), "rests3": ("rests", 1), "ring2": ("ring", 1), "own3": ("pull_own", 0), "reserved4": ("pull_reserved", 0)}


def swap_hand_cases():
    """The hand cases of the rule's branches (coordinates padded as in expert_ref)."""
    c = {}
    # agent 0 behind agent 1, both bound for the right end: agent 1 moves away for its neighbour's swap (step 3 of swap_agent)
    c["clear2"] = dict(grids=er._parse(sr._SWAP_GRID), pos=er._cells([(1, 1), (1, 2)]), goal=er._cells([(1, 5), (1, 4)]), seed=3)
    # agent 2 comes to rest in the pocket (a dead end, its goal): count leaves it out
    c["rests3"] = dict(grids=er._parse(sr._SWAP_GRID), pos=er._cells([(1, 1), (1, 2), (1, 3)]), goal=er._cells([(1, 2), (1, 1), (2, 3)]), seed=3)
    # a closed ring of eight cells, no junction: possible walks back to its origin and gives false
    c["ring2"] = dict(grids=er._parse(_RING), pos=er._cells([(1, 1), (1, 2)]), goal=er._cells([(1, 1), (2, 1)]), seed=3)
    # agent 1 stands where its distance is largest (the far side of a ring): its reversed list starts with its own cell, so nobody is pulled
    c["own3"] = dict(grids=er._parse(_RING_SPUR), pos=er._cells([(1, 1), (1, 2), (1, 3)]), goal=er._cells([(1, 1), (3, 4), (1, 3)]), seed=3)
    # agent 0 pushes agent 1 off the junction, agent 1's swap agent 2 stands in the stub: agent 1's cell is already agent 0's, no pull
    c["reserved4"] = dict(grids=er._parse(_STUB), pos=er._cells([(2, 1), (2, 2), (1, 2), (2, 3)]),
                          goal=er._cells([(2, 4), (1, 2), (2, 1), (2, 3)]), seed=2)
    for v in c.values():
        v.update(n_inst=1, n_agents=v["pos"].shape[1], inst_offset=0, steps=12)
    return c


def maze_case(n_agents=16, n_inst=4, steps=128, seed=7):
    """The dataset's 21 x 21 maze, padded: instance i places its agents with seed 100 + i."""
    from mapf_gpt_amd import maps
    grid = maps.pad(maps.maze_map(21, 21, 7))
    pos = np.empty((n_inst, n_agents, 2), np.int16)
    goal = np.empty((n_inst, n_agents, 2), np.int16)
    for i in range(n_inst):
        pos[i], goal[i] = maps.place_agents(grid, n_agents, 100 + i)
    return dict(grids=grid[None], n_inst=n_inst, n_agents=n_agents, pos=pos, goal=goal, steps=steps, seed=seed, inst_offset=0)


def hand_cases():
    """expert_search_ref.hand_cases() (pocket, rotation, dead_end, swap2, swap3) plus the rule's own."""
    c = sr.hand_cases()
    c.update(swap_hand_cases())
    return c


MAX_ITERS = 256


def gpu_cases():
    """The shapes of tests/test_gpu_expert_swap.py, each with the search's max_iters."""
    c = hand_cases()
    g = er.gpu_cases()
    c["one_agent"] = g["one_agent"]
    c["agents65"] = g["agents65"]          # the first counts at which the loops stride past one wave
    c["agents70"] = g["agents70"]
    c["grids3"], c["shared5"], c["offset7"] = g["grids3"], g["shared5"], g["offset7"]
    c["maze16"] = maze_case()
    for v in c.values():
        v["max_iters"] = MAX_ITERS
    return c
