"""Shapes and expected values of the lifelong batched episode tokenizer's tests, on top of tests/episode_rows_ref.py:
seeded target lists for its random-walk episodes, the rows per kept episode from the pinned restatement (oracle/dataset_oracle.py with
lifelong_targets=), and the base case with the conditions on its data that keep the tests from going empty."""
import numpy as np

from oracle import dataset_oracle as dso
from tests import episode_rows_ref as rr

_cache = {}


def paths_of(init_e, actions_e, length):
    """int64 [n_agents, length + 1, 2]: the cells of one episode's agents."""
    return np.asarray(dso.agent_paths(np.asarray(init_e).astype(int).tolist(), [row[:length].tolist() for row in np.asarray(actions_e)]), np.int64)


def random_targets(grid, init, actions, lengths, seed, within=None):
    """-> int16 [n_batch, n_agents, L = cap + 2, 2].  One np.random.Generator(PCG64(seed)), episodes then agents; per agent: k =
    integers(0, 4); min(k, len + 1) distinct timesteps of 0 .. len by choice(replace=False), sorted: the path's cells at those times are
    the first targets (an agent that follows its path stands on them in this order, unless a fill cell or a repeat comes between);
    uniformly drawn free cells fill the list.  A walk advances at most once per path cell, len + 1 <= cap + 1 times: never exhausted.
    within: the fill cells of an agent lie at most this far, per coordinate, from its first cell.  The reference's encoder has no token
    for a relative goal beyond +-20 (encoder.cpp:93 throws, and so does the restatement), so on a map wider than 21 cells a test keeps
    every goal that far from every observer: within + cap + 5 <= 20."""
    n_batch, n_agents, cap = np.asarray(actions).shape
    rng = np.random.Generator(np.random.PCG64(seed))
    free = np.argwhere(np.asarray(grid) == 0)
    L = cap + 2
    out = np.empty((n_batch, n_agents, L, 2), np.int16)
    for e in range(n_batch):
        ln = int(lengths[e])
        paths = paths_of(init[e], actions[e], ln)
        for a in range(n_agents):
            k = min(int(rng.integers(0, 4)), ln + 1)
            ts = np.sort(rng.choice(ln + 1, size=k, replace=False))
            out[e, a, :k] = paths[a, ts]
            pool = free if within is None else free[(np.abs(free - paths[a, 0]) <= within).all(1)]
            out[e, a, k:] = pool[rng.integers(0, len(pool), L - k)]
    return out


def expand(targets_a, n):
    """One agent's list as the device addresses it, written out: [target(0), ..., target(n - 1)], entry 0 then the rest cyclically."""
    from mapf_gpt_amd.dataset_tokenizer import target_at
    return [[int(v) for v in target_at(targets_a, j)] for j in range(int(n))]


def episode_rows(grid, init_e, actions_e, length, target_lists, mask_cost2go=False):
    """One episode through the restatement, computed once per distinct input: target_lists = per agent a plain list of cells.
    -> (rows uint8 [n_agents * (length + 1), 256], labels int8).  IndexError where the reference raises it."""
    key = (np.asarray(grid).tobytes(), np.asarray(grid).shape, np.asarray(init_e).tobytes(), np.asarray(actions_e)[:, :length].tobytes(),
           int(length), repr([[tuple(int(v) for v in c) for c in tg] for tg in target_lists]), bool(mask_cost2go))
    if key not in _cache:
        made = [row[:length].tolist() for row in np.asarray(actions_e)]
        x, y = dso.generate_observations(grid, np.asarray(init_e).astype(int).tolist(), made, lifelong_targets=target_lists,
                                         mask_cost2go=mask_cost2go)
        x, y = np.asarray(x).astype(np.int8).view(np.uint8).reshape(-1, 256), np.asarray(y).astype(np.int8)
        x.setflags(write=False)
        y.setflags(write=False)
        _cache[key] = (x, y)
    return _cache[key]


def expected(grid, init, actions, lengths, targets, n_targets=None, keep=None, episodes=None, mask_cost2go=False):
    """-> (rows uint8 [N, 256], labels int8 [N], row0 int64 [n_sel + 1]) of tokenize_episodes(..., targets=, n_targets=)."""
    n_batch, n_agents, max_steps = np.asarray(actions).shape
    acts, lens = rr.clamped(actions, lengths, max_steps)
    L = np.asarray(targets).shape[2]
    sel = list(range(n_batch)) if episodes is None else [int(e) for e in episodes]
    xs, ys, row0 = [np.zeros((0, 256), np.uint8)], [np.zeros((0,), np.int8)], [0]
    for e in sel:
        if keep is None or keep[e]:
            lists = [expand(targets[e][a], L if n_targets is None else n_targets[e][a]) for a in range(n_agents)]
            x, y = episode_rows(grid, init[e], acts[e], int(lens[e]), lists, mask_cost2go)
            xs.append(x)
            ys.append(y)
            row0.append(row0[-1] + len(x))
        else:
            row0.append(row0[-1])
    return np.concatenate(xs), np.concatenate(ys), np.asarray(row0, np.int64)


def goal_stats(grid, init, actions, lengths, targets):
    """What the target lists do to the batch: (goal changes after t = 0, agents whose list advances at t = 0, (agent, timestep) pairs
    whose goal is not the path's last cell), from oracle.dataset_oracle.goal_positions."""
    changes = at0 = off_last = 0
    for e in range(len(lengths)):
        paths = paths_of(init[e], actions[e], int(lengths[e]))
        lists = [expand(tg, len(tg)) for tg in targets[e]]
        goals = np.asarray(dso.goal_positions([[tuple(c) for c in p] for p in paths.tolist()], lists), np.int64)
        for a in range(len(paths)):
            at0 += int((goals[a, 0] != np.asarray(lists[a][0])).any())          # (three more advance onto a repeat of the same cell)
            changes += int((goals[a, 1:] != goals[a, :-1]).any(-1).sum())
            off_last += int((goals[a] != paths[a, -1]).any(-1).sum())
    return changes, at0, off_last


def base_case():
    """maps.random_map(9, 11, 0.2, 5) padded, 6 episodes x 7 agents, cap 6, lengths 6, 1, 0, 3, 6, 2, walk seed 1, target seed 101:
    29 goal changes after t = 0, 18 agents that advance at t = 0, 127 of 168 (agent, timestep) pairs off the path's last cell, and every
    row of episode 0 differs from the static-goal row.  The conditions asserted here hold for map seeds 5 and 7 x walk seeds 1-3 (27-32
    changes, 15-24 advances): a regression of the generator cannot empty the tests."""
    if "base" not in _cache:
        from mapf_gpt_amd import maps
        grid = maps.pad(maps.random_map(9, 11, 0.2, 5))
        lengths = [6, 1, 0, 3, 6, 2]
        init, actions = rr.random_walks(grid, 6, 7, 6, lengths, seed=1)
        targets = random_targets(grid, init, actions, lengths, seed=101)
        changes, at0, off_last = goal_stats(grid, init, actions, lengths, targets)
        assert changes >= 20 and at0 >= 5, (changes, at0)
        lists0 = [expand(tg, len(tg)) for tg in targets[0]]
        moving = episode_rows(grid, init[0], actions[0], 6, lists0)[0]
        static = rr.episode_rows(grid, init[0], actions[0], 6)[0]
        differ = int((moving != static).any(1).sum())
        assert differ >= 1
        _cache["base"] = dict(grid=grid, init=init, actions=actions, lengths=lengths, targets=targets,
                              stats=dict(changes=changes, at0=at0, off_last=off_last, differ=differ))
    return _cache["base"]
