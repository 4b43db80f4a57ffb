"""Plain Python restatement of the LaCAM search over the PIBT generator on top of tests/expert_ref.py
(section 20 and the env of section 4) -- TEST INFRASTRUCTURE ONLY, written from the spec, not from the kernel.

    out = search(grid, pos, goal, dist, seed, row0, max_iters, max_steps)     # one instance
    ref = RefSearchExpert(grids, n_inst, n_agents, max_episode_steps, seed, inst_offset, max_iters)
    ref.reset(pos, goal)                   # solves every instance
    actions, planned = ref.step()          # replays the solution of a status-1 instance, plans the others by section 20

`explored` is a dict keyed by the whole configuration: nothing is hashed here.
"""
from collections import deque

import numpy as np

from tests import expert_ref as er

SOLVED, EXHAUSTED, BUDGET, TOO_LONG = 1, 2, 3, 4


class Constraint:
    """(parent constraint, who, k); the root has no parent and depth 0."""
    __slots__ = ("parent", "who", "k", "depth")

    def __init__(self, parent=None, who=None, k=None):
        self.parent, self.who, self.k = parent, who, k
        self.depth = 0 if parent is None else parent.depth + 1

    def chain(self):
        """The (who, k) pairs from the root end."""
        out, c = [], self
        while c.parent is not None:
            out.append((c.who, c.k))
            c = c.parent
        return out[::-1]


class Node:
    def __init__(self, Q, since, depth, parent):
        self.Q, self.since, self.depth, self.parent = list(Q), list(since), depth, parent
        self.order = er.priority_order(self.since)
        self.fifo = deque([Constraint()])


def gen(grid, Q, dist, since, order, chain, seed, t, row0, rule=None):
    """Section 20's step on (Q, since) with the constraints of `chain` applied first.  -> (next cells, actions) or None on failure."""
    out = er.gen(grid, Q, dist, since, order, chain, seed, t, row0, rule)
    return None if out is None else out[:2]


def search(grid, pos, goal, dist, seed, row0, max_iters, max_steps, rule=None):
    """Depth-first LaCAM of one instance over gen(..., rule).  -> dict(status, iters, nodes, length, solution): solution int8
    [n][length] for status 1 and 4, None otherwise; length 0 unless solved."""
    n = len(pos)
    H, W = grid.shape
    goal = [(int(g[0]), int(g[1])) for g in goal]
    start = Node([(int(p[0]), int(p[1])) for p in pos], [0] * n, 0, None)
    open_, explored = [start], {tuple(start.Q): start}
    iters, nodes, found = 0, 1, None
    while open_ and iters < max_iters:
        iters += 1
        N = open_[-1]
        if N.Q == goal:
            found = N
            break
        if not N.fifo:
            open_.pop()
            continue
        C = N.fifo.popleft()
        if C.depth < n:
            i = N.order[C.depth]
            for k, (dr, dc) in enumerate(er.MOVES):
                u = (N.Q[i][0] + dr, N.Q[i][1] + dc)
                if 0 <= u[0] < H and 0 <= u[1] < W and grid[u] == 0 and int(dist[i][u]) != er.UNREACHED:
                    N.fifo.append(Constraint(C, i, k))
        out = gen(grid, N.Q, dist, N.since, N.order, C.chain(), seed, N.depth, row0, rule)
        if out is None:
            continue
        Q2 = out[0]
        if tuple(Q2) in explored:
            continue
        M = Node(Q2, [0 if Q2[a] == goal[a] else N.since[a] + 1 for a in range(n)], N.depth + 1, N)
        explored[tuple(Q2)] = M
        open_.append(M)
        nodes += 1
    if found is None:
        return dict(status=EXHAUSTED if not open_ else BUDGET, iters=iters, nodes=nodes, length=0, solution=None)
    path = []
    while found is not None:
        path.append(found.Q)
        found = found.parent
    path = path[::-1]
    L = len(path) - 1
    sol = np.zeros((n, L), np.int8)
    for t in range(L):
        for a in range(n):
            d = (path[t + 1][a][0] - path[t][a][0], path[t + 1][a][1] - path[t][a][1])
            sol[a, t] = er.MOVES.index(d)
    return dict(status=SOLVED if L <= max_steps else TOO_LONG, iters=iters, nodes=nodes, length=L, solution=sol, path=path)


class RefSearchExpert(er.RefExpert):
    """RefExpert whose reset() solves every instance; step() replays the solution of a status-1 instance and plans the others."""

    def __init__(self, grids, n_inst, n_agents, max_episode_steps, seed=0, inst_offset=0, max_iters=4096):
        super().__init__(grids, n_inst, n_agents, max_episode_steps, seed, inst_offset)
        self.max_iters = int(max_iters)

    def reset(self, pos, goal):
        super().reset(pos, goal)
        n = self.n_agents
        self.found = [search(self.grid(i), self.pos[i], self.goal[i], self.dist[i], self.seed, (self.inst_offset + i) * n,
                             self.max_iters, self.max_steps, self.rule) for i in range(self.n_inst)]

    def stats(self):
        """-> status, iterations, nodes, length: int32 [inst] each."""
        return tuple(np.asarray([f[k] for f in self.found], np.int32) for k in ("status", "iters", "nodes", "length"))

    def solution(self):
        """int8 [inst, agent, max_steps]: the actions of the status-1 instances, zero elsewhere."""
        out = np.zeros((self.n_inst, self.n_agents, self.max_steps), np.int8)
        for i, f in enumerate(self.found):
            if f["status"] == SOLVED:
                out[i, :, :f["length"]] = f["solution"]
        return out

    def plan_instance(self, i):
        f = self.found[i]
        if f["status"] != SOLVED:
            return super().plan_instance(i)
        t = int(self.tcount[i])
        act = [int(f["solution"][a, t]) if t < f["length"] else 0 for a in range(self.n_agents)]
        return [(int(p[0]) + er.MOVES[k][0], int(p[1]) + er.MOVES[k][1]) for p, k in zip(self.pos[i], act)], act


# ---- the shapes both test files use -------------------------------------------------------------------------------------------
_SWAP_GRID = ["#######", "#.....#", "###.###", "#######"]


def hand_cases():
    """expert_ref.hand_cases() plus the two corridor swaps (coordinates padded the same way)."""
    c = er.hand_cases()
    # two agents exchange the ends of a five-cell corridor with one pocket in the middle
    c["swap2"] = dict(grids=er._parse(_SWAP_GRID), pos=er._cells([(1, 1), (1, 5)]), goal=er._cells([(1, 5), (1, 1)]), steps=32)
    c["swap3"] = dict(grids=er._parse(_SWAP_GRID), pos=er._cells([(1, 1), (1, 2), (1, 5)]), goal=er._cells([(1, 5), (1, 4), (1, 1)]), steps=48)
    for k in ("swap2", "swap3"):
        c[k].update(n_inst=1, n_agents=c[k]["pos"].shape[1], seed=3, inst_offset=0)
    return c


# max_iters per shape of tests/test_gpu_expert_search.py
MAX_ITERS = {"agents65": 2048, "agents70": 256}


def gpu_cases():
    """The shapes of tests/test_gpu_expert_search.py: expert_ref.gpu_cases() plus the swaps, each with its max_iters."""
    c = er.gpu_cases()
    c.update({k: v for k, v in hand_cases().items() if k not in c})
    c["agents65"]["steps"] = 64            # the search's solution has 62 steps (PIBT alone does not solve it in 256)
    for k, v in c.items():
        v["max_iters"] = MAX_ITERS.get(k, 512)
    return c


def run_case(case, steps=None, max_iters=None):
    ref = RefSearchExpert(case["grids"], case["n_inst"], case["n_agents"], case["steps"], case["seed"], case["inst_offset"],
                          case.get("max_iters", 512) if max_iters is None else max_iters)
    ref.reset(case["pos"], case["goal"])
    ref.run(case["steps"] if steps is None else steps)
    return ref
