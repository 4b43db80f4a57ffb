"""Plain Python restatement of the refinement pass (single-agent space-time replanning of a found solution) on
top of tests/expert_search_ref.py (section 21) and tests/expert_swap_ref.py (section 22), both imported unchanged -- TEST INFRASTRUCTURE
ONLY, written from the spec, not from the kernels.

    out = refine(grid, path, goal, max_rounds)            # one instance: path = the configurations P[0..L] of a found solution
    out = refine_found(grid, found, goal, max_rounds, horizon, max_steps)      # on search()'s result; the final result in the same shape
    ref = RefRefineExpert(..., max_iters, swap, max_rounds, horizon)
    ref.reset(pos, goal)                   # searches, then refines
    actions, planned = ref.step()          # replays the refined solution of a final-status-1 instance, plans the others by section 20

Everything here works on sets of cells; nothing is packed into words.
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


def path_actions(P):
    n, L = len(P[0]), len(P) - 1
    sol = np.zeros((n, L), np.int8)
    for t in range(L):
        for a in range(n):
            sol[a, t] = er.MOVES.index((P[t + 1][a][0] - P[t][a][0], P[t + 1][a][1] - P[t][a][1]))
    return sol


def refine_found(grid, found, goal, max_rounds, horizon, max_steps):
    """Refine search()'s result `found`.  -> a dict of the same shape with the final status, length, solution and path, plus
    first_status, first_length, soc_before, soc_after, rounds, replans (all 0 but the first two for an instance that is left as it is:
    status 2 or 3, or a solution longer than the horizon)."""
    out = dict(found, first_status=found["status"], first_length=found["length"], soc_before=0, soc_after=0, rounds=0, replans=0)
    if found["status"] not in (sr.SOLVED, sr.TOO_LONG) or found["length"] > horizon:
        return out
    r = refine(grid, found["path"], goal, max_rounds)
    out.update(status=sr.SOLVED if r["length"] <= max_steps else sr.TOO_LONG, length=r["length"], path=r["path"],
               solution=path_actions(r["path"]), soc_before=r["soc_before"], soc_after=r["soc_after"], rounds=r["rounds"],
               replans=r["replans"])
    return out


REFINE_KEYS = ("first_status", "first_length", "soc_before", "soc_after", "rounds", "replans")


class RefRefineExpert(sw.RefSwapSearchExpert):
    """RefSwapSearchExpert whose reset() refines what the search found; step() replays by the final status."""

    def __init__(self, grids, n_inst, n_agents, max_episode_steps, seed=0, inst_offset=0, max_iters=4096, swap=False, max_rounds=16,
                 horizon=None):
        super().__init__(grids, n_inst, n_agents, max_episode_steps, seed, inst_offset, max_iters, swap)
        self.max_rounds, self.horizon = int(max_rounds), 2 * self.max_steps if horizon is None else int(horizon)

    def reset(self, pos, goal):
        super().reset(pos, goal)
        self.first = self.found
        if self.max_rounds > 0:
            self.found = [refine_found(self.grid(i), f, self.goal[i], self.max_rounds, self.horizon, self.max_steps)
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
