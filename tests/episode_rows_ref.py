"""Shapes and expected values of the batched episode tokenizer's tests: seeded random-walk episodes on a padded
grid, their rows per kept episode from the pinned restatement (oracle/dataset_oracle.py), offsets and row order from the rules of
include/mapf_gpt_amd.h stated here a second time."""
import numpy as np

from oracle import dataset_oracle as dso

MOVES = ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1))
_cache = {}


def random_walks(grid, n_batch, n_agents, max_steps, lengths, seed):
    """-> init int16 [n_batch, n_agents, 2], actions int8 [n_batch, n_agents, max_steps] (0 beyond an episode's length): every agent
    starts on a free cell and draws a move per step; a move into an obstacle becomes a wait.  Agents may overlap: the tokenizer does not
    care."""
    rng = np.random.Generator(np.random.PCG64(seed))
    free = np.argwhere(np.asarray(grid) == 0)
    init = free[rng.integers(0, len(free), (n_batch, n_agents))].astype(np.int16)
    actions = np.zeros((n_batch, n_agents, max_steps), np.int8)
    for e in range(n_batch):
        pos = init[e].astype(np.int64)
        for t in range(int(lengths[e])):
            for a in range(n_agents):
                v = int(rng.integers(0, 5))
                r, c = pos[a, 0] + MOVES[v][0], pos[a, 1] + MOVES[v][1]
                if grid[r, c]:
                    v = 0
                else:
                    pos[a] = (r, c)
                actions[e, a, t] = v
    return init, actions


def clamped(actions, lengths, max_steps):
    """The log as the device reads it: bytes outside 0..4 are waits, lengths are cut to [0, max_steps]."""
    a = np.asarray(actions).astype(np.int64)
    return np.where((a >= 0) & (a <= 4), a, 0).astype(np.int8), np.clip(np.asarray(lengths, np.int64), 0, max_steps)


def episode_rows(grid, init_e, actions_e, length, mask_cost2go=False):
    """One episode through the restatement, computed once per distinct input: -> (rows uint8 [n_agents * (length + 1), 256], labels int8)."""
    key = (np.asarray(grid).tobytes(), np.asarray(grid).shape, np.asarray(init_e).tobytes(), np.asarray(actions_e)[:, :length].tobytes(),
           int(length), bool(mask_cost2go))
    if key not in _cache:
        made = [row[:length].tolist() for row in np.asarray(actions_e)]
        x, y = dso.generate_observations(grid, np.asarray(init_e).astype(int).tolist(), made, mask_cost2go=mask_cost2go)
        x, y = np.asarray(x).astype(np.int8).view(np.uint8).reshape(-1, 256), np.asarray(y).astype(np.int8)
        x.setflags(write=False)
        y.setflags(write=False)
        _cache[key] = (x, y)
    return _cache[key]


def expected(grid, init, actions, lengths, keep=None, episodes=None, mask_cost2go=False):
    """-> (rows uint8 [N, 256], labels int8 [N], row0 int64 [n_sel + 1]) of tokenize_episodes on the same arguments."""
    n_batch, n_agents, max_steps = np.asarray(actions).shape
    acts, lens = clamped(actions, lengths, max_steps)
    sel = list(range(n_batch)) if episodes is None else [int(e) for e in episodes]
    xs, ys, row0 = [np.zeros((0, 256), np.uint8)], [np.zeros((0,), np.int8)], [0]
    for e in sel:
        if keep is None or keep[e]:
            x, y = episode_rows(grid, init[e], acts[e], int(lens[e]), mask_cost2go)
            assert len(x) == n_agents * (int(lens[e]) + 1)
            xs.append(x)
            ys.append(y)
            row0.append(row0[-1] + len(x))
        else:
            row0.append(row0[-1])
    return np.concatenate(xs), np.concatenate(ys), np.asarray(row0, np.int64)


def most_agents_in_a_window(init, actions, lengths):
    """The largest number of agents, the observer included, inside any observer's 11 x 11 window over every episode and timestep of the
    (clamped) log.  The kernels keep 128 candidates per window: a case at or below that is one the restatement and the kernels agree on."""
    most = 0
    for e, length in enumerate(lengths):
        made = [row[:int(length)].tolist() for row in np.asarray(actions[e])]
        paths = np.asarray(dso.agent_paths(np.asarray(init[e]).astype(int).tolist(), made), np.int64)      # [n_agents, length + 1, 2]
        near = (np.abs(paths[:, None] - paths[None, :]) <= 5).all(-1)                                      # [observer, agent, timestep]
        most = max(most, int(near.sum(1).max()))
    return most


# Crowded windows at three 64-lane candidate passes, the last one partial: the shared neighbour loop against the restatement.
CROWDED = dict(h=30, w=34, density=0.15, lengths=[3, 2], n_agents=(129, 150))


def crowded_case(n_agents):
    """-> (grid, init, actions, lengths, most agents in a window) of a CROWDED case; the windows hold more agents than a row has slots."""
    from mapf_gpt_amd import maps
    key = ("crowded", n_agents)
    if key not in _cache:
        c = CROWDED
        grid = maps.pad(maps.random_map(c["h"], c["w"], c["density"], 300 + n_agents))
        init, actions = random_walks(grid, 2, n_agents, 3, c["lengths"], seed=n_agents)
        most = most_agents_in_a_window(init, actions, c["lengths"])
        assert most > 13, most
        _cache[key] = (grid, init, actions, list(c["lengths"]), most)
    return _cache[key]


# ---- BatchedExpert.dataset_rows: two maps of different size in one common frame ----------------------------------------------------
# Chosen with tests/expert_ref.py on the CPU (RefExpert, plain PIBT, seed 4) over map seeds {21, 31, 41} x placement seeds {200, 300} x
# caps {8, 10, 12, 16}: (21, 200, 12) is the first with a solved and an unsolved episode and a solved one on either map -- CSR
# [0, 1, 1, 1], lengths [12, 12, 12, 8] (DESIGN.md section 33 has the table).
ROWS_CASE = dict(map_seed=21, place_seed=200, cap=12, n_inst=4, n_agents=6, seed=4, csr=[0, 1, 1, 1], lengths=[12, 12, 12, 8])


def rows_case():
    """-> dict(obst: the two maps' own obstacle arrays, names, grids [2, H, W]: both in their common frame, pos, goal [4, 6, 2])."""
    from mapf_gpt_amd import evaluation as ev
    from mapf_gpt_amd import maps
    c = ROWS_CASE
    obst = [maps.random_map(10, 10, 0.2, c["map_seed"]), maps.random_map(8, 12, 0.2, c["map_seed"] + 1)]
    frames = ev.common_frame([(o, o == 0, o == 0) for o in obst])
    grids = np.stack([f[0] for f in frames])
    pos = np.empty((c["n_inst"], c["n_agents"], 2), np.int16)
    goal = np.empty_like(pos)
    for i in range(c["n_inst"]):
        pos[i], goal[i] = maps.place_agents(grids[i % 2], c["n_agents"], c["place_seed"] + i)
    return dict(obst=obst, names=["random-a", "random-b"], grids=grids, pos=pos, goal=goal)


def map_string(obst):
    return "\n".join("".join("#" if v else "." for v in row) for row in obst)
