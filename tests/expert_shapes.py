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


def assert_not_idle(ref):
    log, lens = ref.log()
    moves = log != 0                                            # [inst, agent, T]; zero beyond an instance's length
    assert (lens > 0).all() and moves.any(axis=(1, 2)).all(), "an instance never moves"
    assert moves.any(axis=(0, 1))[:int(lens.max())].all(), "a step at which every live agent waits"


# ---- more than 192 agents, and the PIBT stack at its full depth (tests/test_expert_many_cpu.py, tests/test_gpu_expert_many.py) ------
# The cases are made once (many_cases()), their distance fields once per case (fields(), by the C oracle's BFS) and shared by every
# mode's restatement through RefExpert.fields; start() is the one place that builds a restatement of them.
LANE_W = 31
LANE_SIZES = (65, 193, 300)                                     # every mode; LANE_BIG for the plan kernel and the shield only
LANE_BIG = 1024
AGENT_CASES = ("agents193", "agents256", "agents257", "agents1024")


def lane(cells):
    """A closed lane one cell wide of exactly `cells` cells, folded left and right every LANE_W cells (one gap cell between two rows),
    padded.  -> (grid, the lane's cells in order, unpadded)."""
    path, r = [], 0
    while len(path) < cells:
        cols = list(range(LANE_W)) if r % 4 == 0 else list(range(LANE_W - 1, -1, -1))
        path += [(r, c) for c in cols] + [(r + 1, cols[-1])]
        r += 2
    path = path[:cells]
    rows = [["#"] * (max(c for _, c in path) + 1) for _ in range(max(r for r, _ in path) + 1)]
    for r, c in path:
        rows[r][c] = "."
    return er._parse(["".join(row) for row in rows]), path


def _lane_case(grid, path, n, goal):
    return dict(grids=grid[None], n_inst=1, n_agents=n, pos=er._cells(path[:n]), goal=er._cells(goal), steps=3, seed=3, inst_offset=0,
                max_iters=64, path=path)


def lane_full(n):
    """n cells, every one with an agent (agent a on cell a).  Agent 0 is bound for the far end, the last agent for cell 0, the others
    stand on their goals: the push of agent 0 runs through all n agents and fails back, every agent waits."""
    grid, path = lane(n)
    return _lane_case(grid, path, n, [path[n - 1]] + path[1:n - 1] + [path[0]])


def lane_shift(n):
    """n + 1 cells, the far one free, every agent bound for the next cell: the push of agent 0 runs through all n agents and succeeds,
    all n move in the one step (which ends the episode)."""
    grid, path = lane(n + 1)
    return _lane_case(grid, path, n, path[1:n + 1])


def lane_forward(case):
    """int32 [1, n]: the action that takes agent a to the lane's next cell (0 for an agent on the lane's last cell)."""
    path, n = case["path"], case["n_agents"]
    return np.array([[er.MOVES.index((path[a + 1][0] - path[a][0], path[a + 1][1] - path[a][1])) if a + 1 < len(path) else 0
                      for a in range(n)]], np.int32)


def lane_logits(case):
    """-> (bits uint32 [1, n, 5], first [1, n]): logits that prefer the lane's forward move for every agent (2.0; waiting 1.0, the other
    moves 0.0), with the forward move as the sampled action too."""
    from tests import shield_ref as sh
    fwd = lane_forward(case)
    logits = np.zeros((1, case["n_agents"], 5), np.float32)
    logits[..., 0] = 1.0
    np.put_along_axis(logits, fwd[..., None].astype(np.int64), np.float32(2.0), axis=2)
    return sh.bits_of(logits).copy(), fwd.astype(np.int64)


_MANY = {}


def many_cases():
    """name -> case (made once, read only).  The agent counts past three waves on non-square maps, up to the env's limit; both lanes at
    every size; one case the search solves, for refinement; one lifelong case."""
    if not _MANY:
        from tests import expert_lifelong_ref as lr
        c = _MANY
        c["agents193"] = dict(er.random_case(30, 44, 0.15, 2, 193, 8, seed=25), max_iters=64)    # the fourth pass has one lane
        c["agents256"] = dict(er.random_case(40, 44, 0.15, 1, 256, 8, seed=26), max_iters=64)    # four whole passes
        c["agents257"] = dict(er.random_case(40, 44, 0.15, 1, 257, 8, seed=27), max_iters=64)
        c["agents1024"] = dict(er.random_case(64, 64, 0.10, 1, 1024, 6, seed=28), max_iters=16)  # the env's limit: 16 passes
        for n in LANE_SIZES + (LANE_BIG,):
            c[f"lane_full{n}"], c[f"lane_shift{n}"] = lane_full(n), lane_shift(n)
        # the default horizon of twice the step cap does not fit: 257 layers of 614 bytes on 70 x 70 cells are beyond a workgroup's LDS
        c["refine257"] = dict(er.random_case(60, 60, 0.05, 1, 257, 128, seed=31), max_iters=256, horizon=128)
        c["lifelong257"] = lr.random_case(40, 44, 0.15, 1, 257, 8, seed=29, Q=8)
    return _MANY


_FIELDS = {}


def fields(name):
    """The distance fields [inst][agent] of a case of many_cases(), by the C oracle's BFS (tests/test_gpu_tokenizer.py pins it against
    the device's fields), computed once; the restatement's own bfs agrees on the first, the last and three agents in between."""
    if name not in _FIELDS:
        from oracle import oracle as orc
        case = many_cases()[name]
        n, grids = case["n_agents"], case["grids"]
        out = [[orc.bfs(grids[i % len(grids)], case["goal"][i, a]) for a in range(n)] for i in range(case["n_inst"])]
        for i in range(case["n_inst"]):
            for a in sorted({0, n // 4, n // 2, (3 * n) // 4, n - 1}):
                assert np.array_equal(out[i][a], er.bfs(grids[i % len(grids)], case["goal"][i, a])), (name, i, a)
        _FIELDS[name] = out
    return _FIELDS[name]


class recursion:
    """The restatement's PIBT is recursive with depth n_agents: `with recursion(case)` raises Python's limit for a case that needs it
    and puts it back."""

    def __init__(self, case):
        self.need = 2 * case["n_agents"] + 400

    def __enter__(self):
        import sys
        self.old = sys.getrecursionlimit()
        sys.setrecursionlimit(max(self.old, self.need))

    def __exit__(self, *exc):
        import sys
        sys.setrecursionlimit(self.old)


def start(name, kind="pibt"):
    """The restatement of a case of many_cases() after reset, on the case's shared fields.  kind: one of MODES (the search modes come
    back solved), "refine" / "refine_swap" (refined), "lifelong", "shield" or "shield_lifelong"."""
    from tests import expert_lifelong_ref as lr, expert_refine_ref as rr, expert_swap_ref as sw, shield_lifelong_ref as slr, shield_ref as sh
    case = many_cases()[name]
    args = (case["grids"], case["n_inst"], case["n_agents"], case["steps"])
    seeded = args + (case["seed"], case["inst_offset"])
    if kind in MODES:
        m = MODES[kind]
        ref = sw.RefSwapSearchExpert(*seeded, case["max_iters"], m["swap"]) if m["search"] else sw.RefSwapExpert(*seeded, m["swap"])
    elif kind in ("refine", "refine_swap"):
        ref = rr.RefRefineExpert(*seeded, case["max_iters"], kind == "refine_swap", rr.ROUNDS, case["horizon"])
        ref.refine_fn = rr.refine_many                          # (the sets of refine() take minutes at this size)
    elif kind == "lifelong":
        ref = lr.RefLifelongExpert(*seeded, case["swap"])
    else:
        ref = {"shield": sh.RefShield, "shield_lifelong": slr.RefShieldLifelong}[kind](*args)
    ref.fields = fields(name)
    with recursion(case):
        ref.reset(case["pos"], case["goal"], *([case["queue"]] if "lifelong" in kind else []))
    return ref
