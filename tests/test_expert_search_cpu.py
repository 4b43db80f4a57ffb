"""The LaCAM search's spec on the host (tests/expert_search_ref.py): the invariants of every transition of a
solution, the hand cases (corridor swaps that PIBT alone never solves, instances the search proves unsolvable, the iteration budget and
the step cap with their PIBT fallback), the root constraint, the record schema, and the restatement's status, iteration and node counts
on the shapes tests/test_gpu_expert_search.py compares the device against."""
import numpy as np
import pytest

from tests import expert_ref as er
from tests import expert_search_ref as sr
from tests.test_expert_cpu import check_step

CASES = sr.gpu_cases()
_REFS = {}


def solved_ref(name):
    """The restatement after the case's whole episode (computed once, read only)."""
    if name not in _REFS:
        _REFS[name] = sr.run_case(CASES[name])
    return _REFS[name]


def search_one(case, max_iters, max_steps=None, i=0):
    n = case["n_agents"]
    grids = np.asarray(case["grids"])
    grid = grids if grids.ndim == 2 else grids[i % len(grids)]
    dist = [er.bfs(grid, case["goal"][i, a]) for a in range(n)]
    return sr.search(grid, case["pos"][i], case["goal"][i], dist, case["seed"], (case["inst_offset"] + i) * n, max_iters,
                     case["steps"] if max_steps is None else max_steps)


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_transition_of_a_solution_keeps_the_invariants(name):
    case, ref = CASES[name], solved_ref(name)
    for i, f in enumerate(ref.found):
        if f["status"] not in (sr.SOLVED, sr.TOO_LONG):
            continue
        grid, path = ref.grid(i), f["path"]
        assert path[0] == [tuple(int(v) for v in p) for p in case["pos"][i]]
        assert path[-1] == [tuple(int(v) for v in g) for g in case["goal"][i]]
        assert len(path) == f["length"] + 1 and f["solution"].shape == (case["n_agents"], f["length"])
        for t in range(f["length"]):
            act = f["solution"][:, t].tolist()
            check_step(grid, path[t], path[t + 1], act)                # distinct, no swap, no blocked cell, one cell; the oracle's env
            assert er.env_step(grid, path[t], act) == path[t + 1]      # and the restatement's env reproduce it


@pytest.mark.parametrize("name", ["swap2", "swap3"])
def test_the_search_solves_a_corridor_swap_that_pibt_does_not(name):
    case = CASES[name]
    pibt = er.run_case(dict(case, steps=256))
    assert pibt.metrics()[0, 0] == 0.0
    ref = solved_ref(name)
    assert ref.stats()[0].tolist() == [sr.SOLVED]
    assert ref.metrics()[0, 0] == 1.0 and ref.metrics()[0, 4] == ref.found[0]["length"]


def test_unsolvable_instances_empty_the_open_stack():
    f = search_one(CASES["pocket"], 512)                        # the free cells are a four-cell path: the two agents cannot pass
    assert f["status"] == sr.EXHAUSTED and f["length"] == 0 and f["solution"] is None
    closed = dict(grids=er._parse(["#####", "#...#", "#####"]), pos=er._cells([(1, 1), (1, 3)]), goal=er._cells([(1, 3), (1, 1)]),
                  n_inst=1, n_agents=2, steps=16, seed=3, inst_offset=0)
    f = search_one(closed, 512)
    assert f["status"] == sr.EXHAUSTED and f["iters"] < 512


def test_a_spent_budget_falls_back_to_the_plain_pibt_episode():
    case = CASES["dead_end"]
    ref = sr.run_case(case, max_iters=64)
    assert [s.tolist() for s in ref.stats()] == [[sr.BUDGET], [64], [1], [0]]
    pibt = er.run_case(case)
    assert np.array_equal(ref.log()[0], pibt.log()[0]) and np.array_equal(ref.log()[1], pibt.log()[1])
    assert np.array_equal(ref.metrics(), pibt.metrics()) and np.array_equal(ref.pos, pibt.pos)


def test_a_solution_longer_than_the_step_cap_falls_back_to_pibt():
    case = dict(CASES["swap2"], steps=6)                        # the search needs 9 steps
    ref = sr.run_case(case)
    st = ref.stats()
    assert st[0].tolist() == [sr.TOO_LONG] and st[3].tolist() == [9] and not ref.solution().any()
    pibt = er.run_case(case)
    assert np.array_equal(ref.log()[0], pibt.log()[0]) and np.array_equal(ref.metrics(), pibt.metrics())


@pytest.mark.parametrize("name", ["rotation", "pocket", "agents70", "shared5"])
def test_with_the_root_constraint_the_generator_is_the_pibt_step(name):
    case = CASES[name]
    ref = er.run_case(case, steps=0)
    for t in range(min(case["steps"], 12)):
        for i in range(case["n_inst"]):
            if ref.done[i]:
                continue
            row0 = (case["inst_offset"] + i) * case["n_agents"]
            want = er.plan(ref.grid(i), ref.pos[i], ref.dist[i], ref.since[i], ref.seed, ref.t, row0)[:2]
            Q = [tuple(int(v) for v in p) for p in ref.pos[i]]
            got = sr.gen(ref.grid(i), Q, ref.dist[i], ref.since[i], er.priority_order(ref.since[i]), [], ref.seed, ref.t, row0)
            assert got == want
        ref.step()


def test_a_constraint_fixes_its_agent_or_fails_the_generator():
    case = CASES["pocket"]                                      # agents on (1,1) and (1,3) of #...# with a pocket under (1,3)
    grid = np.asarray(case["grids"])
    dist = [er.bfs(grid, case["goal"][0, a]) for a in range(2)]
    Q = [tuple(int(v) for v in p) for p in case["pos"][0]]
    run = lambda chain: sr.gen(grid, Q, dist, [0, 0], [0, 1], chain, 3, 0, 0)
    nxt, act = run([(1, 2)])                                    # agent 1 down into the pocket: agent 0 advances
    assert act == [4, 2] and nxt[1] == (Q[1][0] + 1, Q[1][1])
    assert run([(0, 4), (1, 3)]) is None                        # both into the middle cell: reserved
    nxt, act = run([(0, 0)])                                    # agent 0 waits: agent 1 takes the middle
    assert act == [0, 3]
    Q = [(Q[0][0], Q[0][1] + 1), Q[1]]                          # now adjacent: (1,2) and (1,3)
    assert run([(0, 4), (1, 3)]) is None                        # a swap
    assert run([(0, 4), (1, 0)]) is None                        # into a reserved cell (the chain's order does not matter)
    assert run([(1, 0), (0, 4)]) is None


def test_records_of_solved_episodes_go_through_the_dataset_tokenizer():
    from mapf_gpt_amd import dataset_tokenizer as dt
    case, ref = CASES["shared5"], solved_ref("shared5")
    keys = [{"map_name": "m", "seed": i, "num_agents": case["n_agents"]} for i in range(case["n_inst"])]
    recs = er.records(ref, keys, case["pos"], algorithm="LaCAM")
    assert ref.stats()[0].tolist() == [sr.SOLVED] * 5
    for i, r in enumerate(recs):
        m = r["metrics"]
        assert r["algorithm"] == "LaCAM" and m["CSR"] == 1.0 and int(m["ep_length"]) == ref.found[i]["length"]
        paths = dt.agent_paths(m["init_positions"], m["made_actions"])
        labels = dt.gt_actions(m["made_actions"])
        assert paths.shape == (case["n_agents"], ref.found[i]["length"] + 1, 2) and all(len(g) == paths.shape[1] for g in labels)
        assert np.array_equal(paths[:, -1], case["goal"][i])
        assert np.array_equal(paths.transpose(1, 0, 2), np.asarray(ref.found[i]["path"]))


# what the restatement gives on the shapes of tests/test_gpu_expert_search.py: name -> (status, iterations, nodes, length) per instance
PINNED = {
    "pocket": ([2], [62], [6], [0]),
    "rotation": ([1], [2], [2], [1]),
    "dead_end": ([3], [512], [1], [0]),
    "swap2": ([1], [19], [10], [9]),
    "swap3": ([1], [21], [13], [12]),
    "one_agent": ([1], [4], [4], [3]),
    "agents65": ([1], [70], [63], [62]),
    "agents70": ([3], [256], [125], [0]),
    "grids3": ([4, 1, 1], [113, 20, 10], [54, 20, 10], [53, 19, 9]),
    "shared5": ([1, 1, 1, 1, 1], [22, 16, 15, 20, 19], [19, 16, 15, 20, 19], [18, 15, 14, 19, 18]),
    "offset7": ([4, 1, 1], [132, 19, 15], [60, 19, 15], [59, 18, 14]),
}
# solved episodes (CSR = 1) with the search in front, next to tests/test_expert_cpu.py's SOLVED for PIBT alone
SOLVED = {"pocket": 0, "rotation": 1, "dead_end": 0, "swap2": 1, "swap3": 1, "one_agent": 1, "agents65": 1, "agents70": 0, "grids3": 3,
          "shared5": 5, "empty32": 32, "offset7": 3}


def test_status_iteration_and_node_counts_of_the_gpu_shapes():
    assert set(CASES) == set(SOLVED) and set(PINNED) == set(SOLVED) - {"empty32"}
    for name in sorted(CASES):
        ref = solved_ref(name)
        st = [s.tolist() for s in ref.stats()]
        if name == "empty32":                                   # 32 instances: every one solved, a node per iteration, one step less
            assert st[0] == [1] * 32 and st[1] == st[2] and st[3] == [v - 1 for v in st[1]]
        else:
            assert tuple(st) == PINNED[name], (name, st)
        assert int(ref.metrics()[:, 0].sum()) == SOLVED[name], name
