"""Direct oracle-vs-reference comparison along seeded walks.  The reference tokenizer's rows for every step of every walk are
stored under tests/golden/refwalk_*.npz (tests/golden/make_golden_refwalk.py records them with the reference build in
oracle/_ref); the test replays the same inputs through the C oracle and needs nothing outside the repository."""
import os

import numpy as np
import pytest

from mapf_gpt_amd import maps
from oracle import oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RANDOM_CASES = [(20, 21, 0.15, 24, 1), (30, 90, 0.25, 30, 2), (70, 66, 0.3, 20, 3), (130, 40, 0.1, 16, 4), (64, 64, 0.35, 40, 5)]
CORNER_SEEDS = [0, 1, 2]
CORNER_SITES = [(128, 128), (128, 192), (192, 128), (192, 192)]


def random_walk(h, w, dens, n, seed):
    """A random map and 10 steps of random actions -> grid, [(pos, goal, last actions)] fed to update_agents at each step."""
    grid = maps.pad(maps.random_map(h, w, dens, seed))
    pos, goal = maps.place_agents(grid, n, seed)
    rng = np.random.Generator(np.random.PCG64(seed))
    p, g, last = pos.astype(np.int32), goal.astype(np.int32), np.full(n, -1, np.int32)
    steps = []
    for t in range(10):
        steps.append((p.copy(), g.copy(), last.copy()))
        last = rng.integers(0, 5, n).astype(np.int32)
        p, _ = orc.env_step(grid, p, g, last)
    return grid, steps


def corner_walk(seed):
    """Maps larger than 128 in both dimensions: agents wander around the (left + 123, top + 123) spots of their cached
    partial windows, where the reference's unseeded window corner (cpp:178-198) is in view -> grid, steps, corner-spot hits."""
    rng = np.random.Generator(np.random.PCG64(500 + seed))
    grid = maps.pad((rng.random((220, 230)) < 0.1).astype(np.uint8))
    for cr, cc in CORNER_SITES:
        grid[cr - 9: cr + 3, cc - 9: cc + 3] = (rng.random((12, 12)) < 0.08)
    comp = maps.largest_component(grid == 0)
    n = 24
    starts = []
    for k in range(n):                                         # starts inside the windows whose corner is the site
        cr, cc = CORNER_SITES[k % 4]
        for _ in range(10000):
            p = (int(cr - 5 - rng.integers(0, 4)), int(cc - 5 - rng.integers(0, 4)))
            if comp[p] and p not in starts:
                starts.append(p)
                break
        else:
            raise AssertionError("no free start cell near the corner site")
    free = np.argwhere(comp)
    goal = free[rng.integers(0, len(free), n)].astype(np.int32)
    goal[:8] = free[np.argsort(-(free.sum(1)))[:8]]            # some goals beyond every corner
    first = np.array([(p[0] - 60, p[1] - 60) for p in starts], np.int32)     # created with the origin the site belongs to
    for k in range(n):
        if not comp[tuple(first[k])]:
            d = np.abs(free - first[k]).sum(1)
            first[k] = free[d.argmin()]
    p, last = first.copy(), np.full(n, -1, np.int32)
    steps, hits = [], 0
    for t in range(40):
        if t == 1:
            p = np.array(starts, np.int32)                     # positions are inputs: a jump into the corner region
        if t == 20:
            goal[8:16] = free[rng.integers(0, len(free), 8)]   # goal changes reset the window origin (cpp:464-468)
        steps.append((p.copy(), goal.copy(), last.copy()))
        hits += sum(1 for a in range(n) if any(p[a][0] + 5 == cr and p[a][1] + 5 == cc for cr, cc in CORNER_SITES))
        last = rng.integers(0, 5, n).astype(np.int32)
        bias = rng.random(n) < 0.5                             # drift towards the spot: down / right
        last[bias] = rng.choice([2, 4], bias.sum())
        p, _ = orc.env_step(grid, p, goal, last)
    return grid, steps, hits


def random_name(h, w, dens, n, seed):
    return f"refwalk_random_{h}x{w}_s{seed}"


def corner_name(seed):
    return f"refwalk_corner_s{seed}"


def _replay_against_reference(name, grid, steps):
    ref = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert np.array_equal(ref["grid"], grid), f"{name}: the walk's map is not the one the reference rows were recorded on"
    mine = orc.OracleGenerator(grid)
    assert ref["tokens"].shape[0] == len(steps)
    for t, (p, g, last) in enumerate(steps):
        assert np.array_equal(ref["pos"][t], p) and np.array_equal(ref["goal"][t], g) and np.array_equal(ref["actions"][t], last), \
            f"{name} step {t}: the walk's inputs are not the ones the reference rows were recorded on"
        if t == 0:
            mine.create_agents(p, g)
        mine.update_agents(p, g, last)
        want, got = ref["tokens"][t], mine.generate_observations()
        assert np.array_equal(want, got), f"{name} step {t}: rows {np.argwhere((want != got).any(1)).ravel().tolist()}"


@pytest.mark.parametrize("h,w,dens,n,seed", RANDOM_CASES)
def test_random_maps_bit_exact(h, w, dens, n, seed):
    grid, steps = random_walk(h, w, dens, n, seed)
    _replay_against_reference(random_name(h, w, dens, n, seed), grid, steps)


@pytest.mark.parametrize("seed", CORNER_SEEDS)
def test_partial_window_corner_walks(seed):
    """Recompute rule and corner value must follow the reference step by step near the partial windows' corners (ADVICE r1:
    plain BFS differs there)."""
    grid, steps, hits = corner_walk(seed)
    assert hits > 0, "no agent ever stood on a corner-view spot"
    _replay_against_reference(corner_name(seed), grid, steps)
