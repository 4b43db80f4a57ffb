"""Plain Python / numpy restatement of the PIBT expert's spec together with the env spec (DESIGN.md
section 4) -- TEST INFRASTRUCTURE ONLY, written from the two specs, not from the kernels.

    ref = RefExpert(grids, n_inst, n_agents, max_episode_steps, seed, inst_offset)
    ref.reset(pos, goal)
    actions, planned = ref.step()          # int32 [inst, agent], int16 [inst, agent, 2]

State after any number of steps: ref.pos, ref.since, ref.done, ref.log() and ref.metrics().
"""
from collections import deque

import numpy as np

MOVES = ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1))      # 0 wait, 1 up, 2 down, 3 left, 4 right
UNREACHED = 65535
M64 = (1 << 64) - 1
DENSITY_RADIUS = 5


def splitmix_z(seed, step, row):
    """The sampler's 64-bit value for (seed, step, global row) before its final shift (mapf_gpt_amd/sampling.py)."""
    z = (seed + 0x9E3779B97F4A7C15 * (step + 1)) & M64
    z ^= (row * 0xD1342543DE82EF95) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def bfs(grid, goal):
    """4-connected distance-to-goal field, uint16, 65535 = wall or unreached."""
    H, W = grid.shape
    d = np.full((H, W), UNREACHED, np.int64)
    gr, gc = int(goal[0]), int(goal[1])
    if grid[gr, gc] == 0:
        d[gr, gc] = 0
        q = deque([(gr, gc)])
        while q:
            r, c = q.popleft()
            for dr, dc in MOVES[1:]:
                rr, cc = r + dr, c + dc
                if 0 <= rr < H and 0 <= cc < W and grid[rr, cc] == 0 and d[rr, cc] == UNREACHED:
                    d[rr, cc] = d[r, c] + 1
                    q.append((rr, cc))
    return d.astype(np.uint16)


def priority_order(since):
    """Agents by (since desc, id asc)."""
    return sorted(range(len(since)), key=lambda a: (-int(since[a]), a))


def candidates(grid, pos, dist, occ_now, seed, t, row0, a):
    """Agent a's candidates (key, action, cell) by ascending key."""
    H, W = grid.shape
    z = splitmix_z(seed, t, row0 + a)
    out = []
    for k, (dr, dc) in enumerate(MOVES):
        u = (pos[a][0] + dr, pos[a][1] + dc)
        if not (0 <= u[0] < H and 0 <= u[1] < W) or grid[u] != 0:
            continue
        d = int(dist[a][u])
        if d == UNREACHED:
            continue
        o = 1 if (u in occ_now and occ_now[u] != a) else 0
        r = (z >> (5 * k)) & 31
        out.append(((((d * 2 + o) * 32 + r) * 8 + k), k, u))
    return sorted(out)


class _Fail(Exception):
    pass


def gen(grid, Q, dist, since, order, chain, seed, t, row0, rule=None):
    """The configuration generator: section 20's step on the cells Q, agents taken in `order`, with the (agent, action) constraints
    of `chain` applied first (section 21).  `rule`, if given, is called with the state (grid, Q, dist, occ_now, nxt, act, next_occ)
    and returns section 22's rule on it: an object with order(a, C) and pull(a, j, first) (tests/expert_swap_ref.py).
    -> (next cells, actions, deepest stack reached), or None when the generator fails (with a chain only)."""
    n = len(Q)
    Q = [(int(p[0]), int(p[1])) for p in Q]
    occ_now = {p: a for a, p in enumerate(Q)}
    next_occ = {}
    nxt, act, fixed = [None] * n, [0] * n, [False] * n
    rule = rule(grid, Q, dist, occ_now, nxt, act, next_occ) if rule is not None else None
    depth = [0, 0]

    for a, k in chain:
        u = (Q[a][0] + MOVES[k][0], Q[a][1] + MOVES[k][1])
        if u in next_occ:
            return None
        c = occ_now.get(u)
        if c is not None and c != a and nxt[c] is not None and nxt[c] == Q[a]:
            return None
        nxt[a], act[a], fixed[a] = u, k, True
        next_occ[u] = a

    def pibt(a, parent):
        depth[0] += 1
        depth[1] = max(depth[1], depth[0])
        try:
            C, j = candidates(grid, Q, dist, occ_now, seed, t, row0, a), None
            if rule is not None:
                C, j = rule.order(a, C)
            for i, (_, k, u) in enumerate(C):
                if u in next_occ:
                    continue
                if parent is not None and u == Q[parent]:
                    continue
                c = occ_now.get(u)
                if c is not None and nxt[c] is not None and nxt[c] == Q[a]:
                    continue
                nxt[a], act[a] = u, k
                next_occ[u] = a
                if c is not None and c != a and nxt[c] is None:
                    if not pibt(c, a):
                        continue
                if rule is not None:
                    rule.pull(a, j, i == 0)
                return True
            holder = next_occ.get(Q[a])
            if holder is not None and fixed[holder]:
                raise _Fail()
            nxt[a], act[a] = Q[a], 0
            next_occ[Q[a]] = a
            return False
        finally:
            depth[0] -= 1

    try:
        for a in order:
            if nxt[a] is None:
                pibt(a, None)
    except _Fail:
        return None
    return nxt, act, depth[1]


def plan(grid, pos, dist, since, seed, t, row0):
    """One PIBT step of one instance.  pos [n][2], dist [n][H][W], since [n]; row0 = global row of agent 0.
    -> (next cells [n] of (r, c), actions [n], deepest stack reached)."""
    return gen(grid, pos, dist, since, priority_order(since), (), seed, t, row0)


def env_step(grid, pos, actions):
    """The env spec's collision rules (defaults): -> new cells [n] of (r, c)."""
    H, W = grid.shape
    n = len(pos)
    cur = [(int(p[0]), int(p[1])) for p in pos]
    tgt = []
    for a in range(n):
        k = int(actions[a])
        dr, dc = MOVES[k] if 0 <= k <= 4 else (0, 0)
        u = (cur[a][0] + dr, cur[a][1] + dc)
        tgt.append(u if (0 <= u[0] < H and 0 <= u[1] < W and grid[u] == 0) else cur[a])            # 1
    where = {c: a for a, c in enumerate(cur)}
    swap = [tgt[a] != cur[a] and tgt[a] in where and where[tgt[a]] != a and tgt[where[tgt[a]]] == cur[a] for a in range(n)]
    tgt = [cur[a] if swap[a] else tgt[a] for a in range(n)]                                       # 2
    while True:                                                                                   # 3
        claims = {}
        for u in tgt:
            claims[u] = claims.get(u, 0) + 1
        rev = [a for a in range(n) if tgt[a] != cur[a] and claims[tgt[a]] > 1]
        if not rev:
            return tgt
        for a in rev:
            tgt[a] = cur[a]


def density_sample(grid, pos, radius=DENSITY_RADIUS):
    """Mean over the agents of (agents in the (2r+1)^2 window, itself included) / (traversable cells of the window)."""
    H, W = grid.shape
    free = np.zeros((H + 2 * radius, W + 2 * radius), np.int64)
    free[radius:radius + H, radius:radius + W] = grid == 0
    p = np.asarray(pos, np.int64).reshape(-1, 2)
    vals = []
    for r, c in p:
        cnt = int(np.count_nonzero((np.abs(p[:, 0] - r) <= radius) & (np.abs(p[:, 1] - c) <= radius)))
        vals.append(cnt / int(free[r:r + 2 * radius + 1, c:c + 2 * radius + 1].sum()))
    return float(np.mean(vals))


class RefExpert:
    rule = None                                                   # section 22's rule, as gen() takes it (tests/expert_swap_ref.py sets it)
    fields = None                                                 # optional: the distance fields [inst][agent] of reset()'s goals (tests/expert_shapes.py)

    def __init__(self, grids, n_inst, n_agents, max_episode_steps, seed=0, inst_offset=0):
        grids = np.asarray(grids)
        if grids.ndim == 2:
            grids = grids[None]
        self.grids = (grids != 0).astype(np.uint8)
        self.n_inst, self.n_agents, self.max_steps = int(n_inst), int(n_agents), int(max_episode_steps)
        self.seed, self.inst_offset = int(seed) & M64, int(inst_offset)

    def grid(self, i):
        return self.grids[i % len(self.grids)]

    def reset(self, pos, goal):
        n_inst, n = self.n_inst, self.n_agents
        self.pos = np.asarray(pos, np.int64).reshape(n_inst, n, 2).copy()
        self.goal = np.asarray(goal, np.int64).reshape(n_inst, n, 2).copy()
        if self.fields is not None:                               # precomputed for these goals and shared: the lists are copied, not the fields
            self.dist = [list(row) for row in self.fields]
        else:
            self.dist = [[bfs(self.grid(i), self.goal[i, a]) for a in range(n)] for i in range(n_inst)]
        self.since = np.zeros((n_inst, n), np.int64)
        self.done = np.zeros(n_inst, np.uint8)
        self.t = 0
        self.tcount = np.zeros(n_inst, np.int64)
        self.arrive = np.where((self.pos == self.goal).all(-1), 0, -1).astype(np.int64)
        self.dens = [[density_sample(self.grid(i), self.pos[i])] for i in range(n_inst)]
        self.made = [[[] for _ in range(n)] for _ in range(n_inst)]
        self.max_depth = 0

    def plan_instance(self, i):
        """The step of instance i: -> (next cells, actions)."""
        since = self.since[i]
        nxt, act, depth = gen(self.grid(i), self.pos[i], self.dist[i], since, priority_order(since), (), self.seed, self.t,
                              (self.inst_offset + i) * self.n_agents, self.rule)
        self.max_depth = max(self.max_depth, depth)
        return nxt, act

    def step(self):
        n_inst, n = self.n_inst, self.n_agents
        actions = np.zeros((n_inst, n), np.int32)
        planned = self.pos.astype(np.int16).copy()                # a done instance plans to stay where it is
        for i in range(n_inst):
            if self.done[i]:
                continue
            grid = self.grid(i)
            nxt, act = self.plan_instance(i)
            actions[i], planned[i] = act, np.asarray(nxt, np.int16)
            for a in range(n):
                self.made[i][a].append(int(act[a]))
            was_on = (self.pos[i] == self.goal[i]).all(-1)
            self.pos[i] = np.asarray(env_step(grid, self.pos[i], act), np.int64)
            self.tcount[i] += 1
            on = (self.pos[i] == self.goal[i]).all(-1)
            self.arrive[i] = np.where(on, np.where(was_on, self.arrive[i], self.tcount[i]), -1)
            self.dens[i].append(density_sample(grid, self.pos[i]))
            self.since[i] = np.where(on, 0, self.since[i] + 1)
            if on.all():
                self.done[i] = 1
            elif self.tcount[i] >= self.max_steps:
                self.done[i] = 2
        self.t += 1
        return actions, planned

    def run(self, steps):
        for _ in range(steps):
            self.step()

    def log(self):
        """-> (made_actions int8 [inst, agent, max_steps], zero beyond an instance's length; lengths int32 [inst])."""
        out = np.zeros((self.n_inst, self.n_agents, self.max_steps), np.int8)
        for i in range(self.n_inst):
            for a in range(self.n_agents):
                m = self.made[i][a]
                out[i, a, :len(m)] = m
        return out, np.asarray([len(self.made[i][0]) for i in range(self.n_inst)], np.int32)

    def metrics(self):
        """float64 [inst, 6] = CSR, ISR, SoC, makespan, ep_length, avg_agents_density (env spec)."""
        out = np.zeros((self.n_inst, 6))
        for i in range(self.n_inst):
            t = int(self.tcount[i])
            on = (self.pos[i] == self.goal[i]).all(-1)
            ta = np.where(on, np.maximum(self.arrive[i], 0), t)
            out[i] = (float(on.all()), on.sum() / self.n_agents, ta.sum(), ta.max(), t, float(np.mean(self.dens[i])))
        return out


def records(ref, run_keys, init_pos, algorithm="PIBT"):
    """The toolbox record shape of BatchedExpert.records, from the restatement's state."""
    keys = ("CSR", "ISR", "SoC", "makespan", "ep_length", "avg_agents_density")
    m = ref.metrics()
    out = []
    for i in range(ref.n_inst):
        rec = {k: float(m[i, j]) for j, k in enumerate(keys)}
        rec["made_actions"] = [list(a) for a in ref.made[i]]
        rec["init_positions"] = np.asarray(init_pos[i]).astype(int).tolist()
        out.append({"metrics": rec, "env_grid_search": dict(run_keys[i]), "algorithm": algorithm})
    return out


# ---- the shapes both test files use -------------------------------------------------------------------------------------------
PAD = 5


def _parse(rows):
    return np.pad(np.array([[1 if ch == "#" else 0 for ch in r] for r in rows], np.uint8), PAD, constant_values=1)


def _cells(cells):
    return np.asarray(cells, np.int16).reshape(1, -1, 2) + PAD


def hand_cases():
    """name -> dict(grids, n_inst, n_agents, pos, goal, steps, seed).  Coordinates are padded."""
    c = {}
    # head-on in a corridor of three cells with one pocket under its right end: agent 0 (higher priority by id) pushes agent 1 into the pocket
    c["pocket"] = dict(grids=_parse(["#####", "#...#", "###.#", "#####"]), pos=_cells([(1, 1), (1, 3)]), goal=_cells([(1, 3), (1, 1)]), steps=6)
    # three agents on a 2 x 2 block, each wanting the cell of the next: a chain of inherited priorities, all move at once
    c["rotation"] = dict(grids=_parse(["####", "#..#", "#..#", "####"]), pos=_cells([(1, 1), (1, 2), (2, 2)]),
                         goal=_cells([(1, 2), (2, 2), (2, 1)]), steps=4)
    # a closed lane of eight cells, full: agent 0 wants to cross, the push runs to the far end and fails back
    c["dead_end"] = dict(grids=_parse(["##########", "#........#", "##########"]), pos=_cells([(1, 1 + i) for i in range(8)]),
                         goal=_cells([(1, 8)] + [(1, 1 + i) for i in range(1, 8)]), steps=3)
    for v in c.values():
        v.update(n_inst=1, n_agents=v["pos"].shape[1], seed=3, inst_offset=0)
    return c


def random_case(h, w, density, n_inst, n_agents, steps, seed, n_grids=1, inst_offset=0, map_seed=11):
    from mapf_gpt_amd import maps
    grids = np.stack([maps.pad(maps.random_map(h, w, density, map_seed + g)) for g in range(n_grids)])
    pos = np.empty((n_inst, n_agents, 2), np.int16)
    goal = np.empty((n_inst, n_agents, 2), np.int16)
    for i in range(n_inst):
        pos[i], goal[i] = maps.place_agents(grids[i % n_grids], n_agents, 100 + inst_offset + i)
    return dict(grids=grids, n_inst=n_inst, n_agents=n_agents, pos=pos, goal=goal, steps=steps, seed=seed, inst_offset=inst_offset)


def gpu_cases():
    """The shapes of tests/test_gpu_expert.py (and of the solved counts pinned in tests/test_expert_cpu.py)."""
    c = hand_cases()
    c["one_agent"] = random_case(12, 12, 0.2, 1, 1, 32, seed=1)
    c["agents65"] = random_case(16, 16, 0.2, 1, 65, 32, seed=5)           # the first counts at which the rank and scatter loops
    c["agents70"] = random_case(16, 16, 0.2, 1, 70, 32, seed=6)           # stride past one wave
    c["grids3"] = random_case(12, 12, 0.2, 3, 8, 40, seed=7, n_grids=3)
    c["shared5"] = random_case(12, 12, 0.2, 5, 8, 40, seed=8)
    c["empty32"] = random_case(8, 8, 0.0, 32, 4, 24, seed=9)
    c["offset7"] = random_case(12, 12, 0.2, 3, 8, 40, seed=10, inst_offset=7)
    return c


def run_case(case, steps=None):
    ref = RefExpert(case["grids"], case["n_inst"], case["n_agents"], case["steps"], case["seed"], case["inst_offset"])
    ref.reset(case["pos"], case["goal"])
    ref.run(case["steps"] if steps is None else steps)
    return ref
