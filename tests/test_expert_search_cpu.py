"""The LaCAM search's spec on the host (tests/expert_search_ref.py): the invariants of every transition of a
solution, the hand cases (corridor swaps that PIBT alone never solves, instances the search proves unsolvable, the iteration budget and
the step cap with their PIBT fallback), the root constraint, the record schema, and the restatement's status, iteration and node counts
on the shapes tests/test_gpu_expert_search.py compares the device against."""
import numpy as np
import pytest

from tests import expert_ref as er
from tests import expert_search_ref as sr
from tests.test_expert_cpu import check_step, digest

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


# digests (tests/test_expert_cpu.py: digest, and where they come from): name -> (PIBT alone, the search in front) on the case
DIGESTS = {
    "agents65": ("5d88e9b28816893259aab868c214e8cec1c33ef2a82f95656c00254229f4b118",
        "e4902bd7954763bb222b83e15a6ce161a7c06faf71a3137be11d71e5756c18a1"),
    "agents70": ("f3f8fb4d77b1aa11c57fdf32dc5f5d779e4cc31f692c30693f8ac7ba8c458fee",
        "11dda0a66c69d29ac0512f273ded572adbdb2bc17fbc0fe04cbbab01e327ac89"),
    "dead_end": ("e4ad371d0863106482f2143dae3b48cde24b77ecf7dc2603733460c285541c18",
        "5756673cb3da9c279aa637a5f8d1c4fcc2c7f12ee921fb2d6296aa6c67a00881"),
    "empty32": ("a34b4d0cb2818e427999733db95dc61f26fad075903540fbb08710838ca3c20b",
        "9460ef711f098416f18bda7a7c2f70412eda5164408814498f279d3dbd4f21bf"),
    "grids3": ("bda730317c520112eb9a3b200fc2740b309d3c83a0b5bd962281363293fbeb68",
        "b3d9872a55af0beba99a921aa56b01c08d1aca9d9ec44b3cb6b3f5ecf0f8aa27"),
    "offset7": ("7ff9eb94b377d3862e0fd0dc93947015989b131f7534f9f856d3b472d0299479",
        "c19d06c0f685750593b5d4dff45a3b315aa57df67fb0a00dba937906ffab2f02"),
    "one_agent": ("8ea4d162561388b8d808b7ba214d0dd26f03ca388f1d03f047eb30c273cbdcf9",
        "88d1f05a50ef80492dc0e61bc8f8fc1983762bd3a920b20df77c276c7e03a4cb"),
    "pocket": ("74f400dd2d16e04fc3349ec6ad42f63404151396d68388ba1639d7315038c22f",
        "6edf3eb6adf4b5d4c45550738f0658b1421bc2eb20989f4b089efb713c289e37"),
    "rotation": ("4d169063e2b52792a2e1bf65a51733510d2951d58bdae06e2612182b9d9159d5",
        "1b5b8b9ce97303ce362817d284db3f2dbb3af037c70e311c66168b14339f28d4"),
    "shared5": ("8f580042702ab7131c72494830c6c9c41a55ffae01678a51f3359957ebbf15b1",
        "1c0012d6aaa967d898dd975356043ab8b9a2cd63fe635a15173d6c3845fad8a5"),
    "swap2": ("2e17ab82e026b495a91a74709b86217d634165a5281f27bca3a2a2b210e37605",
        "7c85ed72b36c30fd4ec982e7078746fcaefe518ca6c20711cb3b01ceba6a9ede"),
    "swap3": ("8b0b2a2a2d497c27a0d38ddfaebe85a6adbe7b0b712759ecdc732daa1c8be9e0",
        "303c459e2fdaad02d3b0a3624388d883e0a2eaa640c93b91c09c0d5c12e0c97b"),
}


def test_the_episodes_and_searches_of_the_gpu_shapes_are_bit_for_bit_what_they_were():
    assert set(CASES) == set(DIGESTS)
    assert {name: (digest(er.run_case(CASES[name])), digest(solved_ref(name))) for name in sorted(CASES)} == DIGESTS
