"""Plain Python restatement of the refinement pass (single-agent space-time replanning of a found solution) on
top of tests/expert_search_ref.py (section 21) and tests/expert_swap_ref.py (section 22), both imported unchanged -- TEST INFRASTRUCTURE
ONLY, written from the spec, not from the kernels.

    out = refine(grid, path, goal, max_rounds)            # one instance: path = the configurations P[0..L] of a found solution
    out = refine_found(grid, found, goal, max_rounds, horizon, max_steps)      # on search()'s result; the final result in the same shape
    ref = RefRefineExpert(..., max_iters, swap, max_rounds, horizon)
    ref.reset(pos, goal)                   # searches, then refines
    actions, planned = ref.step()          # replays the refined solution of a final-status-1 instance, plans the others by section 20

Everything here works on sets of cells; nothing is packed into words -- but for refine_many(), refine() again for cases of hundreds of
agents, which keeps a set of cells as one Python integer and is held equal to refine() on the small cases.
"""
import numpy as np

from tests import expert_ref as er
from tests import expert_search_ref as sr
from tests import expert_swap_ref as sw


def arrivals(P, goal):
    """arr(a): the start of agent a's final uninterrupted stay on its goal at time L = len(P) - 1 (0 if it never left it)."""
    L = len(P) - 1
    out = []
    for a, g in enumerate(goal):
        assert P[L][a] == g
        t = L
        while t > 0 and P[t - 1][a] == g:
            t -= 1
        out.append(t)
    return out


def replan(grid, P, goal, a, arr_a):
    """Replan agent a against the others' fixed paths.  -> the new cells of a for t = 0..T (T < arr_a), or None when nothing changes."""
    H, W = grid.shape
    L, g = len(P) - 1, goal[a]
    occ = [{P[t][b]: b for b in range(len(goal)) if b != a} for t in range(L + 1)]
    hold = 0
    for t in range(L + 1):
        if g in occ[t]:
            hold = t + 1

    def exchange(t, u, v):
        """The move u -> v between t and t + 1 swaps cells with the agent standing on v."""
        b = occ[t].get(v)
        return b is not None and occ[t + 1].get(u) == b

    reach, T = [{P[0][a]}], None
    for t in range(arr_a):
        if t >= hold and g in reach[t]:
            T = t
            break
        nxt = set()
        for u in reach[t]:
            for dr, dc in er.MOVES:
                v = (u[0] + dr, u[1] + dc)
                if 0 <= v[0] < H and 0 <= v[1] < W and grid[v] == 0 and v not in occ[t + 1] and not exchange(t, u, v):
                    nxt.add(v)
        reach.append(nxt)
    if T is None:
        return None
    cells, v = [g], g
    for t in range(T, 0, -1):
        for dr, dc in er.MOVES:                                 # wait first
            u = (v[0] - dr, v[1] - dc)
            if u in reach[t - 1] and not exchange(t - 1, u, v):
                break
        else:
            raise AssertionError("a reached cell has no predecessor")
        cells.append(u)
        v = u
    assert v == P[0][a]
    return cells[::-1]


def refine(grid, path, goal, max_rounds):
    """-> dict(path, length, arr, soc_before, soc_after, rounds, replans).  `path` is not modified."""
    n = len(goal)
    goal = [(int(g[0]), int(g[1])) for g in goal]
    P = [[(int(c[0]), int(c[1])) for c in q] for q in path]
    arr = arrivals(P, goal)
    assert max(arr) == len(P) - 1
    soc_before, rounds, replans = sum(arr), 0, 0
    while rounds < max_rounds:
        rounds += 1
        adopted = 0
        for a in range(n):
            if arr[a] == 0:
                continue
            new = replan(grid, P, goal, a, arr[a])
            if new is None:
                continue
            for t in range(len(P)):
                P[t][a] = new[t] if t < len(new) else goal[a]
            arr = arrivals(P, goal)
            assert arr[a] == len(new) - 1
            P = P[:max(arr) + 1]
            adopted += 1
        replans += adopted
        if adopted == 0:
            break
    return dict(path=P, length=len(P) - 1, arr=arr, soc_before=soc_before, soc_after=sum(arr), rounds=rounds, replans=replans)


_BACK = (0, 2, 1, 4, 3)                                          # the move that undoes move k


def refine_many(grid, path, goal, max_rounds):
    """refine() for a case whose sets would take minutes (hundreds of agents on an open map: tests/expert_shapes.py's refine257): the
    same rules and the same result, with a set of cells kept as one Python integer (bit r * W + c) and the others' paths kept per time
    step and updated when a replan is adopted, where replan() forms them again for every agent.  tests/test_expert_many_cpu.py holds
    it equal to refine() on every case of gpu_cases()."""
    H, W = grid.shape
    n = len(goal)
    goal = [(int(g[0]), int(g[1])) for g in goal]
    P = [[(int(c[0]), int(c[1])) for c in q] for q in path]
    bit = lambda c: 1 << (c[0] * W + c[1])
    move = lambda u, v: er.MOVES.index((v[0] - u[0], v[1] - u[1]))
    frame = (1 << (H * W)) - 1
    free = sum(bit((int(r), int(c))) for r, c in np.argwhere(grid == 0))
    first_col, last_col = sum(bit((r, 0)) for r in range(H)), sum(bit((r, W - 1)) for r in range(H))

    def moved(m, k):
        """The cells u + MOVES[k] inside the frame, for the cells u of m."""
        return (m, m >> W, (m << W) & frame, (m & ~first_col) >> 1, (m & ~last_col) << 1)[k]

    # occ[t]: the cells on which an agent stands at t; went[t][k]: the cells at t of the agents that make move k between t and t + 1
    occ = [sum(bit(c) for c in q) for q in P]
    went = [[0] * 5 for _ in range(len(P) - 1)]

    def toggle(a):                                              # takes agent a's path out of occ and went, or puts it in
        for t in range(len(P)):
            occ[t] ^= bit(P[t][a])
            if t + 1 < len(P):
                went[t][move(P[t][a], P[t + 1][a])] ^= bit(P[t][a])

    for t in range(len(P) - 1):
        for a in range(n):
            went[t][move(P[t][a], P[t + 1][a])] |= bit(P[t][a])

    def replan_a(a, arr_a):                                     # with agent a taken out: occ and went are the others'
        g, gb = goal[a], bit(goal[a])
        hold = max([t + 1 for t in range(len(P)) if occ[t] & gb], default=0)
        reach, T = [bit(P[0][a])], None
        for t in range(arr_a):
            if t >= hold and reach[t] & gb:
                T = t
                break
            nxt = 0
            for k in range(5):                                  # u -> v = u + MOVES[k] is an exchange when the agent on v goes to u
                nxt |= moved(reach[t], k) & ~went[t][_BACK[k]]
            reach.append(nxt & free & ~occ[t + 1])
        if T is None:
            return None
        cells, v = [g], g
        for t in range(T, 0, -1):
            for k, (dr, dc) in enumerate(er.MOVES):             # wait first
                u = (v[0] - dr, v[1] - dc)
                if 0 <= u[0] < H and 0 <= u[1] < W and reach[t - 1] & bit(u) and not went[t - 1][_BACK[k]] & bit(v):
                    break
            else:
                raise AssertionError("a reached cell has no predecessor")
            cells.append(u)
            v = u
        assert v == P[0][a]
        return cells[::-1]

    arr = arrivals(P, goal)
    assert max(arr) == len(P) - 1
    soc_before, rounds, replans = sum(arr), 0, 0
    while rounds < max_rounds:
        rounds += 1
        adopted = 0
        for a in range(n):
            if arr[a] == 0:
                continue
            toggle(a)
            new = replan_a(a, arr[a])
            if new is not None:
                for t in range(len(P)):
                    P[t][a] = new[t] if t < len(new) else goal[a]
            toggle(a)
            if new is None:
                continue
            arr = arrivals(P, goal)
            assert arr[a] == len(new) - 1
            P = P[:max(arr) + 1]
            del occ[len(P):], went[len(P) - 1:]
            adopted += 1
        replans += adopted
        if adopted == 0:
            break
    return dict(path=P, length=len(P) - 1, arr=arr, soc_before=soc_before, soc_after=sum(arr), rounds=rounds, replans=replans)


def path_actions(P):
    n, L = len(P[0]), len(P) - 1
    sol = np.zeros((n, L), np.int8)
    for t in range(L):
        for a in range(n):
            sol[a, t] = er.MOVES.index((P[t + 1][a][0] - P[t][a][0], P[t + 1][a][1] - P[t][a][1]))
    return sol


def refine_found(grid, found, goal, max_rounds, horizon, max_steps, refine_fn=None):
    """Refine search()'s result `found`.  -> a dict of the same shape with the final status, length, solution and path, plus
    first_status, first_length, soc_before, soc_after, rounds, replans (all 0 but the first two for an instance that is left as it is:
    status 2 or 3, or a solution longer than the horizon)."""
    out = dict(found, first_status=found["status"], first_length=found["length"], soc_before=0, soc_after=0, rounds=0, replans=0)
    if found["status"] not in (sr.SOLVED, sr.TOO_LONG) or found["length"] > horizon:
        return out
    r = (refine_fn or refine)(grid, found["path"], goal, max_rounds)
    out.update(status=sr.SOLVED if r["length"] <= max_steps else sr.TOO_LONG, length=r["length"], path=r["path"],
               solution=path_actions(r["path"]), soc_before=r["soc_before"], soc_after=r["soc_after"], rounds=r["rounds"],
               replans=r["replans"])
    return out


REFINE_KEYS = ("first_status", "first_length", "soc_before", "soc_after", "rounds", "replans")


class RefRefineExpert(sw.RefSwapSearchExpert):
    """RefSwapSearchExpert whose reset() refines what the search found; step() replays by the final status."""
    refine_fn = None                                            # refine, or refine_many where a test sets it

    def __init__(self, grids, n_inst, n_agents, max_episode_steps, seed=0, inst_offset=0, max_iters=4096, swap=False, max_rounds=16,
                 horizon=None):
        super().__init__(grids, n_inst, n_agents, max_episode_steps, seed, inst_offset, max_iters, swap)
        self.max_rounds, self.horizon = int(max_rounds), 2 * self.max_steps if horizon is None else int(horizon)

    def reset(self, pos, goal):
        super().reset(pos, goal)
        self.first = self.found
        if self.max_rounds > 0:
            self.found = [refine_found(self.grid(i), f, self.goal[i], self.max_rounds, self.horizon, self.max_steps, self.refine_fn)
                          for i, f in enumerate(self.first)]

    def refine_stats(self):
        """-> first status, first length, SoC before, SoC after, rounds, replans: int32 [inst] each."""
        return tuple(np.asarray([f[k] for f in self.found], np.int32) for k in REFINE_KEYS)


def run_case(case, steps=None, swap=False, max_rounds=16, horizon=None, max_iters=None):
    ref = RefRefineExpert(case["grids"], case["n_inst"], case["n_agents"], case["steps"], case["seed"], case["inst_offset"],
                          case.get("max_iters", 512) if max_iters is None else max_iters, swap, max_rounds, horizon)
    ref.reset(case["pos"], case["goal"])
    ref.run(case["steps"] if steps is None else steps)
    return ref


ROUNDS = 16


def gpu_cases():
    """The shapes of both test files: expert_search_ref.gpu_cases() (the hand cases, the swaps, 1, 65 and 70 agents, grids3, shared5,
    empty32, offset7), each with the search's max_iters; every one is run with the swap rule off and on."""
    return sr.gpu_cases()
