"""The cases of tests/test_gpu_expert_many.py on the host, on the restatements alone: what keeps the device tests from passing
vacuously.  Every agent-count case (193, 256, 257 and 1024 agents) is not idle; both lanes drive the restatement's recursion to depth n
at every size, without and with the swap rule and under the shield's preference order; lane_full makes every agent wait, lane_shift
moves all n at once; the search solves refine257 and refinement replans there; the independent checker (tests/expert_checks.py)
accepts every step of every run and its replay reproduces the final cells and metrics.  The distance fields of a case are computed
once (expert_shapes.fields) and shared by all of its runs."""
import numpy as np
import pytest

from tests import expert_checks as ck
from tests import expert_ref as er
from tests import expert_shapes as es
from tests import shield_ref as sh

CASES = es.many_cases()
LANES = [f"{form}{n}" for form in ("lane_full", "lane_shift") for n in es.LANE_SIZES]
BIG_LANES = [f"{form}{es.LANE_BIG}" for form in ("lane_full", "lane_shift")]


def run_checked(name, kind):
    """The whole episode of a case in one of the planner's modes, every step through check_transition, the log through replay."""
    case = CASES[name]
    ref = es.start(name, kind)
    pos0 = ref.pos.copy()
    with es.recursion(case):
        for _ in range(case["steps"]):
            before, skip = ref.pos.copy(), ref.done != 0
            act, planned = ref.step()
            ck.check_transition(case["grids"], before, act, planned, ref.pos, skip)
    log, lens = ref.log()
    final, metrics = ck.replay(case["grids"], pos0, ref.goal, log, lens)
    assert np.array_equal(final, ref.pos)
    assert np.array_equal(metrics, ref.metrics()[:, :5]) and np.array_equal(metrics[:, 4], lens)
    return ref


# 1024 agents: the two ends of the LDS carve, as on the device
AGENT_RUNS = [(name, mode) for name in es.AGENT_CASES for mode in sorted(es.MODES) if name != "agents1024" or mode in ("pibt", "search_swap")]


@pytest.mark.parametrize("name,mode", AGENT_RUNS)
def test_the_agent_count_cases_are_not_idle_and_pass_the_checker(name, mode):
    ref = run_checked(name, mode)
    es.assert_not_idle(ref)
    if es.MODES[mode]["search"]:                                # the search ends at the iteration cap: the episode is the plan kernel's
        status, iters, nodes, _ = ref.stats()
        assert (status == 3).all() and (iters == CASES[name]["max_iters"]).all() and (nodes >= CASES[name]["max_iters"] - 1).all()


def test_the_cases_have_the_shapes_they_are_named_for():
    for name, (n_inst, n) in {"agents193": (2, 193), "agents256": (1, 256), "agents257": (1, 257), "agents1024": (1, 1024),
                              "refine257": (1, 257), "lifelong257": (1, 257)}.items():
        case = CASES[name]
        assert (case["n_inst"], case["n_agents"]) == (n_inst, n) and case["pos"].shape == (n_inst, n, 2)
        assert len({tuple(p) for p in case["pos"][0].tolist()}) == n           # one agent per cell
    H, W = CASES["agents193"]["grids"].shape[1:]
    assert H != W
    for n in es.LANE_SIZES + (es.LANE_BIG,):
        full, shift = CASES[f"lane_full{n}"], CASES[f"lane_shift{n}"]
        assert int((full["grids"] == 0).sum()) == n and int((shift["grids"] == 0).sum()) == n + 1
        for case in (full, shift):                              # one cell wide and closed: two ends of degree 1, degree 2 between them
            free = case["grids"][0] == 0
            deg = sum(np.roll(free, s, axis) for s in (1, -1) for axis in (0, 1))[free]
            assert sorted(deg.tolist()) == [1, 1] + [2] * (int(free.sum()) - 2)
            assert case["n_agents"] == n and (case["pos"][0, 0] == er._cells([case["path"][0]])[0, 0]).all()


@pytest.mark.parametrize("name", LANES + BIG_LANES)
def test_a_lane_drives_the_stack_to_depth_n(name):
    case, n = CASES[name], CASES[name]["n_agents"]
    ref = es.start(name, "pibt")
    with es.recursion(case):
        act, planned = ref.step()
    assert ref.max_depth == n
    if name.startswith("lane_full"):                            # the push fails back: every agent waits
        assert (act == 0).all() and np.array_equal(planned, case["pos"]) and ref.done[0] == 0
    else:                                                       # the push succeeds: all n move, and stand on their goals
        assert np.array_equal(act, es.lane_forward(case)) and (act != 0).all() and ref.done[0] == 1
        assert np.array_equal(ref.pos, case["goal"])
    if n == es.LANE_BIG:                                        # the limit is back where it was
        import sys
        assert sys.getrecursionlimit() < 2 * n


# what the swap rule does on the lanes: it never fires.  lane_full: agent 0's swap with agent 1 is required (the
# walk runs the lane's whole length to the dead end) but not possible (no junction behind agent 0); every other agent's best candidate is
# its own cell, or its neighbour is decided.  lane_shift: no agent's neighbour wants to come the other way.  The stack still reaches n.
@pytest.mark.parametrize("name", LANES)
def test_with_the_swap_rule_the_stack_still_reaches_depth_n(name):
    case, n = CASES[name], CASES[name]["n_agents"]
    ref = es.start(name, "pibt_swap")
    with es.recursion(case):
        act, _ = ref.step()
    assert ref.max_depth == n
    assert not {"swap", "clear", "pull", "cap"} & set(ref.trace), ref.trace
    plain = es.start(name, "pibt")
    with es.recursion(case):
        assert np.array_equal(act, plain.step()[0])


@pytest.mark.parametrize("name", LANES + BIG_LANES)
def test_under_the_shields_preference_order_a_lane_reaches_depth_n(name):
    case, n = CASES[name], CASES[name]["n_agents"]
    bits, first = es.lane_logits(case)
    ref = es.start(name, "shield")
    with es.recursion(case):
        _, act, depth = er.gen(ref.grid(0), ref.pos[0], ref.dist[0], ref.since[0], er.priority_order(ref.since[0]), (), 0, 0, 0,
                               sh.make_rule(first[0], bits[0]))
        before = ref.pos.copy()
        got, planned = ref.step(bits, first)
    assert depth == n and np.array_equal(got[0], act)
    ck.check_transition(case["grids"], before, got, planned, ref.pos, np.zeros(1, bool))
    if name.startswith("lane_full"):
        assert (got == 0).all() and ref.overrides[0] == n - 1   # every agent but the last was sampled a move
        with es.recursion(case):                                # and again with agent 0 and the last one ahead in the order
            assert (ref.step(bits, first)[0] == 0).all() and ref.overrides[0] == 2 * (n - 1)
    else:
        assert np.array_equal(got, first) and ref.overrides[0] == 0 and ref.done[0] == 1


@pytest.mark.parametrize("mode", ["pibt_swap", "search", "search_swap"])
@pytest.mark.parametrize("name", LANES)
def test_the_lanes_pass_the_checker_in_every_mode(name, mode):
    ref = run_checked(name, mode)
    if es.MODES[mode]["search"]:
        got = [int(x[0]) for x in ref.stats()]                  # status, iterations, nodes, length
        # lane_shift: the root's first successor is the goal.  lane_full has no solution and one configuration: every one of the cap's 64
        # iterations runs the generator through the whole lane (under another constraint) and finds the root again
        assert got == ([1, 2, 2, 1] if name.startswith("lane_shift") else [3, 64, 1, 0])


@pytest.mark.parametrize("name", LANES + BIG_LANES)
def test_the_plain_lanes_pass_the_checker(name):
    run_checked(name, "pibt")


@pytest.mark.parametrize("kind", ["refine", "refine_swap"])
def test_refine257_is_solved_and_refinement_replans(kind):
    ref = run_checked("refine257", kind)
    first_status, first_length, soc_before, soc_after, rounds, replans = (int(x[0]) for x in ref.refine_stats())
    assert first_status == 1 and ref.first[0]["iters"] <= CASES["refine257"]["max_iters"] and first_length <= CASES["refine257"]["horizon"]
    assert replans >= 1 and rounds >= 1 and soc_after < soc_before
    assert int(ref.stats()[0][0]) == 1 and int(ref.stats()[3][0]) <= first_length
    assert ref.done[0] == 1                                     # the refined solution, replayed, ends the episode solved


def test_refine_many_equals_refine_on_the_small_cases():
    """refine257 runs on refine_many (integers as sets of cells); here it gives refine()'s result, paths included, on every solution the
    search finds on the shapes of expert_refine_ref.gpu_cases(), without and with the swap rule."""
    from tests import expert_refine_ref as rr
    compared = adopted = 0
    for swap in (False, True):
        for name, case in sorted(rr.gpu_cases().items()):
            ref = rr.run_case(case, steps=0, swap=swap, max_rounds=0)
            for i, f in enumerate(ref.found):
                if f["status"] in (1, 4):
                    want = rr.refine(ref.grid(i), f["path"], ref.goal[i], rr.ROUNDS)
                    assert rr.refine_many(ref.grid(i), f["path"], ref.goal[i], rr.ROUNDS) == want, (name, swap, i)
                    compared, adopted = compared + 1, adopted + want["replans"]
    assert compared >= 40 and adopted >= 100


def test_the_lifelong_case_arrives_and_passes_the_checker():
    case = CASES["lifelong257"]
    ref = es.start("lifelong257", "lifelong")
    for _ in range(case["steps"]):
        before = ref.pos.copy()
        act, planned = ref.step()
        ck.check_transition(case["grids"], before, act, planned, ref.pos, np.zeros(1, bool))
    assert ref.arrivals_log().sum() >= 1 and len(set(ref.arrivals[0])) > 1       # the per-step sums are not all alike
    shared = es.fields("lifelong257")[0]                        # an arrival replaces the agent's field in the run's own list only
    assert sum(f is not g for f, g in zip(shared, ref.dist[0])) == len(np.flatnonzero(ref.reached[0]))
    assert all(np.array_equal(shared[a], er.bfs(case["grids"][0], case["goal"][0, a])) for a in np.flatnonzero(ref.reached[0]))


@pytest.mark.parametrize("name", ["agents193", "agents257", "agents1024"])
def test_the_shield_cases_override_and_pass_the_checker(name):
    case = CASES[name]
    ref = es.start(name, "shield")
    rng = np.random.default_rng(case["seed"])
    for _ in range(case["steps"]):
        bits = sh.random_logits(rng, case["n_inst"], case["n_agents"])
        first = rng.integers(0, 5, size=(case["n_inst"], case["n_agents"]))
        before, skip = ref.pos.copy(), ref.done != 0
        act, planned = ref.step(bits, first)
        ck.check_transition(case["grids"], before, np.where(skip[:, None], 0, act), planned, ref.pos, skip)
    assert (ref.overrides > 0).all() and (ref.pos != case["pos"]).any()


def test_the_lifelong_shield_case_arrives_and_overrides():
    from tests import shield_lifelong_ref as slr
    case = CASES["lifelong257"]
    ref = es.start("lifelong257", "shield_lifelong")
    rng = np.random.default_rng(slr.SEED)
    for t in range(case["steps"]):
        before = ref.pos.copy()
        act, planned = ref.step(*slr.step_inputs(ref, rng, t))
        ck.check_transition(case["grids"], before, act, planned, ref.pos, np.zeros(1, bool))
    assert ref.reached.sum() >= 1 and ref.overrides[0] >= 1
