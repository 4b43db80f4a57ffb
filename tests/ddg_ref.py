"""Plain Python restatement of the delta data generation spec -- TEST INFRASTRUCTURE ONLY, written from the spec:
the pick over integer tables, `moves` from positions, and the probe and the teacher by running the expert restatements
(tests/expert_ref.py and the swap, search and refine restatements, unchanged) one snapshot at a time under the stated global ids.
"""
import numpy as np

from tests import expert_ref as er
from tests import expert_refine_ref as rf
from tests import expert_swap_ref as sw


def n_snapshots(T, every):
    return T // every + 1


def valid_table(lengths, T, every):
    return [[j * every <= int(L) for j in range(n_snapshots(T, every))] for L in lengths]


def pick(valid, solved, cost, min_delta=None):
    """Per instance: (picked, j*, delta*) -- candidates j have j and j + 1 valid and j solved; the smallest j of the largest
    cost[j + 1] - cost[j]; picked iff a candidate exists and (min_delta is None or delta* >= min_delta); (False, 0, 0) otherwise."""
    out = []
    for v, s, c in zip(valid, solved, cost):
        best = None
        for j in range(len(v) - 1):
            if v[j] and v[j + 1] and s[j]:
                d = int(c[j + 1]) - int(c[j])
                if best is None or d > best[1]:
                    best = (j, d)
        if best is None or (min_delta is not None and best[1] < min_delta):
            out.append((False, 0, 0))
        else:
            out.append((True, best[0], best[1]))
    return out


def moves(path):
    """path [T + 1][n][2] -> [n][T]: the k with path[t] + MOVES[k] == path[t + 1] (0 for an agent that stayed)."""
    path = np.asarray(path, np.int64)
    out = [[] for _ in range(path.shape[1])]
    for t in range(path.shape[0] - 1):
        for a in range(path.shape[1]):
            d = (int(path[t + 1, a, 0] - path[t, a, 0]), int(path[t + 1, a, 1] - path[t, a, 1]))
            assert d in er.MOVES, f"agent {a} jumped at step {t}"
            out[a].append(er.MOVES.index(d))
    return out


def make_expert(kw, grid, n_agents, steps, seed, gid):
    """The restatement of BatchedExpert(grid, 1, n_agents, steps, seed=seed, inst_offset=gid, **kw)."""
    kw = dict(kw)
    search, swap = kw.pop("search", None), bool(kw.pop("swap", False))
    max_iters, rounds, horizon = kw.pop("max_iters", 4096), kw.pop("refine_rounds", 0), kw.pop("refine_horizon", None)
    assert not kw, f"keywords the restatement does not know: {sorted(kw)}"
    if search == "lacam":
        return rf.RefRefineExpert(grid, 1, n_agents, steps, seed, gid, max_iters, swap, rounds, horizon)
    assert search is None and not rounds
    return sw.RefSwapExpert(grid, 1, n_agents, steps, seed, gid, swap=True) if swap else er.RefExpert(grid, 1, n_agents, steps, seed, gid)


def episode(kw, grid, pos, goal, steps, seed, gid):
    ref = make_expert(kw, grid, len(pos), steps, seed, gid)
    ref.reset(np.asarray(pos)[None], np.asarray(goal)[None])
    ref.run(steps)
    return ref


def collect(grids, pos_traj, lengths, goal, run_keys, every, probe, teacher, probe_steps=None, teacher_steps=None, min_delta=None,
            seed=0, global_ids=None, max_episode_steps=None):
    """-> dict with the tables and records of mapf_gpt_amd.ddg.collect_from_trajectory (lists and numpy)."""
    grids = np.asarray(grids)
    if grids.ndim == 2:
        grids = grids[None]
    pos_traj, goal = np.asarray(pos_traj, np.int64), np.asarray(goal, np.int64)
    T, n_inst, n_agents = pos_traj.shape[0] - 1, pos_traj.shape[1], pos_traj.shape[2]
    J = n_snapshots(T, every)
    cap = max_episode_steps or T
    probe_steps, teacher_steps = probe_steps or cap, teacher_steps or cap
    gids = list(range(n_inst)) if global_ids is None else [int(g) for g in global_ids]
    valid = valid_table(lengths, T, every)
    solved = [[False] * J for _ in range(n_inst)]
    cost = [[0] * J for _ in range(n_inst)]
    probed = 0
    for i in range(n_inst):
        grid = grids[i % len(grids)]
        for j in range(J):
            if not valid[i][j]:
                continue
            snap = pos_traj[j * every, i]
            if (snap == goal[i]).all():
                solved[i][j] = True
                continue
            probed += 1
            m = episode(probe, grid, snap, goal[i], probe_steps, seed, gids[i] * J + j).metrics()[0]
            solved[i][j] = m[0] == 1
            cost[i][j] = int(m[2]) if solved[i][j] else n_agents * (probe_steps + 1)
    picks = pick(valid, solved, cost, min_delta)
    records, teacher_metrics = [], []
    for i, (ok, j, d) in enumerate(picks):
        if not ok:
            continue
        snap = pos_traj[j * every, i]
        ref = episode(teacher, grids[i % len(grids)], snap, goal[i], teacher_steps, seed, gids[i])
        key = dict(run_keys[i])
        key["ddg_step"], key["ddg_delta"] = j * every, d
        records.extend(er.records(ref, [key], snap[None], algorithm="DDG"))
        teacher_metrics.append(ref.metrics()[0])
    return {"records": records, "valid": np.asarray(valid), "solved": np.asarray(solved), "cost": np.asarray(cost, np.int64),
            "picked": np.asarray([p[0] for p in picks]), "j": np.asarray([p[1] for p in picks], np.int64),
            "dmax": np.asarray([p[2] for p in picks], np.int64), "teacher_metrics": np.asarray(teacher_metrics).reshape(-1, 6), "probed": probed}


# ---- the shapes the test files share -------------------------------------------------------------------------------------------
def walk(grid, pos, actions):
    """The env restatement along hand-written actions [T][n] -> path int64 [T + 1, n, 2]."""
    path = [np.asarray(pos, np.int64)]
    for act in actions:
        path.append(np.asarray(er.env_step(grid, path[-1], act), np.int64))
    return np.stack(path)


def hand_trajectory():
    """An empty 8 x 8 grid, 3 agents, K = 4, T = 16.  Agent a starts at (2a, 0) with its goal at (2a + 3, 7), ten steps away.  It walks
    toward the goal for two segments (seven cells right, one down), away from it in the third (up, then three cells left), and back in
    the fourth (three right, one down): the cost-to-go falls, falls, rises and falls again, so the largest delta is at j = 2.  Nobody
    stands on a goal at the end, so the episode runs its 16 steps.
    -> dict(grids, pos_traj [17, 1, 3, 2], lengths [1], goal [1, 3, 2], run_keys, every, T)."""
    grid = er._parse(["........"] * 8)
    pos = er._cells([(0, 0), (2, 0), (4, 0)])[0]
    goal = er._cells([(3, 7), (5, 7), (7, 7)])[0]
    one = [4] * 7 + [2] + [1] + [3] * 3 + [4] * 3 + [2]
    path = walk(grid, pos, [[k] * 3 for k in one])
    assert len(one) == 16 and not (path[-1] == goal).all(-1).any()
    return dict(grids=grid, pos_traj=path[:, None], lengths=np.array([16]), goal=goal[None].astype(np.int16),
                run_keys=[{"map_name": "empty8", "seed": 0, "num_agents": 3}], every=4, T=16)


def random_walk(grid, pos, goal, T, seed):
    """A stand-in for an untrained policy's episode: uniform random actions through the env restatement, ended as the env ends it (every
    agent on its goal, or T steps).  -> (path int64 [T + 1, n, 2] with the last cell repeated beyond the end, length)."""
    rng = np.random.default_rng(seed)
    path, length = [np.asarray(pos, np.int64)], T
    for t in range(T):
        path.append(np.asarray(er.env_step(grid, path[-1], rng.integers(0, 5, len(pos))), np.int64))
        if (path[-1] == np.asarray(goal)).all():
            length = t + 1
            break
    while len(path) < T + 1:
        path.append(path[-1])
    return np.stack(path), length


# tests/test_gpu_ddg.py's tiny-policy batch: 4 instances x 6 agents on a 10 x 10 map at 20 % obstacles, T = 24, K = 8
POLICY_CASE = dict(h=10, w=10, density=0.2, n_inst=4, n_agents=6, T=24, every=8, map_seed=11, seed=3)
