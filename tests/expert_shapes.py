"""The shapes of tests/test_gpu_expert_shapes.py -- TEST INFRASTRUCTURE ONLY: what expert_ref.gpu_cases() and its two descendants leave
out.  Agent counts at and past the wave boundaries (64, 128, 129, 192) on non-square maps, the dataset's named maps with the recipe's
placement, a distance-to-goal beyond a byte, and a map without the wall border, where the in-frame test of the kernels decides.

Every case is a dict as expert_ref.random_case() makes it, plus `max_iters` for the search modes.
"""
import numpy as np

from tests import expert_ref as er


def named_case(name, n_inst, n_agents, steps, seed, max_iters, first_seed=100):
    """A named map with agents placed as runner.make_instances places them: instance i by maps.place_agents(..., first_seed + i)."""
    from mapf_gpt_amd import maps
    grid, s_ok, g_ok = maps.load_named(name)
    comp = maps.largest_component(grid == 0)
    pos = np.empty((n_inst, n_agents, 2), np.int16)
    goal = np.empty((n_inst, n_agents, 2), np.int16)
    for i in range(n_inst):
        pos[i], goal[i] = maps.place_agents(grid, n_agents, first_seed + i, s_ok, g_ok, component=comp)
    return dict(grids=grid[None], n_inst=n_inst, n_agents=n_agents, pos=pos, goal=goal, steps=steps, seed=seed, inst_offset=0,
                max_iters=max_iters)


SERPENTINE_ROWS, SERPENTINE_W = 17, 21


def serpentine():
    """One corridor of 17 lanes of 21 cells folded left and right (373 cells) with one pocket off cell 20, padded.  -> (grid, the corridor's cells in order)."""
    rows, path = [], []
    for lane in range(SERPENTINE_ROWS):
        cols = list(range(SERPENTINE_W)) if lane % 2 == 0 else list(range(SERPENTINE_W - 1, -1, -1))
        rows.append("." * SERPENTINE_W + (".#" if lane == 0 else "##"))          # one pocket, right of the first lane's end
        path += [(2 * lane, c) for c in cols]
        if lane + 1 < SERPENTINE_ROWS:
            gap = cols[-1]
            rows.append("#" * gap + "." + "#" * (SERPENTINE_W + 1 - gap))
            path.append((2 * lane + 1, gap))
    return er._parse(rows), path


def serpentine_case():
    """Four agents in the corridor, all past the pocket: agent 0 walks from cell 23 to cell 363 (distance 340 > 255), agent 1 comes
    the other way from cell 30 (with the swap rule the two go back to the pocket: the rule's walks run over 300 cells and read
    distances beyond a byte), agent 2 walks ahead of them from distance 262, so that its distance passes from 256 to 255 within the
    episode (a planner that read one byte of it would stop there), agent 3 walks back from the far end."""
    grid, path = serpentine()
    at = lambda *idx: er._cells([path[i] for i in idx])
    return dict(grids=grid[None], n_inst=1, n_agents=4, pos=at(23, 30, 50, 372), goal=at(363, 10, 312, 40), steps=24, seed=4, inst_offset=0,
                max_iters=64)


def frame_case():
    """A 9 x 13 map with NO wall border whose free cells touch all four edges: an agent on an edge loses a candidate to the bounds
    test, not to a wall."""
    from mapf_gpt_amd import maps
    grid = maps.random_map(9, 13, 0.15, 21)
    free = grid == 0
    assert free[0].any() and free[-1].any() and free[:, 0].any() and free[:, -1].any()
    n_inst, n_agents = 2, 20
    pos = np.empty((n_inst, n_agents, 2), np.int16)
    goal = np.empty((n_inst, n_agents, 2), np.int16)
    for i in range(n_inst):
        pos[i], goal[i] = maps.place_agents(grid, n_agents, 100 + i)
    return dict(grids=grid[None], n_inst=n_inst, n_agents=n_agents, pos=pos, goal=goal, steps=16, seed=12, inst_offset=0, max_iters=64)


def shape_cases():
    c = {}
    # one, two and three whole waves, and the first count past two: non-square maps, two instances each
    c["agents64"] = er.random_case(20, 23, 0.15, 2, 64, 16, seed=21)
    c["agents128"] = er.random_case(24, 31, 0.2, 2, 128, 16, seed=22, n_grids=2, inst_offset=3)
    c["agents129"] = er.random_case(24, 31, 0.25, 2, 129, 16, seed=23)
    c["agents192"] = er.random_case(30, 44, 0.15, 2, 192, 16, seed=24)
    for k in ("agents64", "agents128", "agents129", "agents192"):
        c[k]["max_iters"] = 64
    # the dataset recipe's maps
    c["maze32"] = named_case("validation-mazes-seed-000", 4, 32, 64, seed=5, max_iters=128)
    c["warehouse192"] = named_case("wfi_warehouse", 1, 192, 24, seed=6, max_iters=64)
    c["berlin24"] = named_case("Berlin_1_256_00", 1, 24, 12, seed=7, max_iters=64)
    c["serpentine"] = serpentine_case()
    c["frame"] = frame_case()
    return c


MODES = {"pibt": dict(search=False, swap=False), "pibt_swap": dict(search=False, swap=True),
         "search": dict(search=True, swap=False), "search_swap": dict(search=True, swap=True)}


def run_mode(case, mode, steps=None):
    """The restatement of a case in one of the four modes, after `steps` steps (default: the case's whole episode)."""
    from tests import expert_swap_ref as sw
    m = MODES[mode]
    return (sw.run_search_case if m["search"] else sw.run_case)(case, steps=steps, swap=m["swap"])
