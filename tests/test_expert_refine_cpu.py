"""The refinement pass's spec on the host (tests/expert_refine_ref.py) on the search's hand cases and
gpu_cases(), with the swap rule off and on, at 16 rounds: the invariants of every transition of a refined solution and its replay
through the oracle's env, per-agent monotonicity, the fixed point, optimality where it can be told (one agent; swap2 against a
brute-force search over joint configurations), the rescues, the round cap, the horizon, statuses 2 and 3, the dataset tokenizer, and
the restatement's statistics on the shapes tests/test_gpu_expert_refine.py compares the device against."""
from collections import deque

import numpy as np
import pytest

from tests import expert_checks as ck
from tests import expert_ref as er
from tests import expert_refine_ref as rr
from tests import expert_search_ref as sr
from tests import expert_swap_ref as sw

CASES = rr.gpu_cases()
_REFS = {}
SWAP = pytest.mark.parametrize("swap", [False, True], ids=["plain", "swap"])


def refined_ref(name, swap=False, **kw):
    """The restatement after the case's whole episode (computed once, read only)."""
    key = (name, swap, tuple(sorted(kw.items())))
    if key not in _REFS:
        _REFS[key] = rr.run_case(CASES[name], swap=swap, **kw)
    return _REFS[key]


def refined(ref):
    """(i, first, final) of the instances the pass took."""
    return [(i, a, b) for i, (a, b) in enumerate(zip(ref.first, ref.found)) if b["rounds"] > 0]


@SWAP
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_transition_of_a_refined_solution_keeps_the_invariants_and_replays(name, swap):
    case, ref = CASES[name], refined_ref(name, swap)
    for i, first, f in refined(ref):
        grid, P, L = ref.grid(i), np.asarray(f["path"]), f["length"]
        assert P.shape == (L + 1, case["n_agents"], 2) and f["solution"].shape == (case["n_agents"], L)
        for t in range(L):
            ck.check_transition(grid, P[t][None], f["solution"][:, t][None], P[t + 1][None], P[t + 1][None], [False])
        log = f["solution"][None] if L else np.zeros((1, case["n_agents"], 1), np.int8)
        final, m = ck.replay(grid, case["pos"][i][None], case["goal"][i][None], log, [L])
        assert np.array_equal(final[0], case["goal"][i])
        assert m[0].tolist() == [1.0, 1.0, float(f["soc_after"]), float(L), float(L)]      # CSR, ISR, SoC, makespan, ep_length
        assert f["status"] == (sr.SOLVED if L <= case["steps"] else sr.TOO_LONG)


@SWAP
@pytest.mark.parametrize("name", sorted(CASES))
def test_no_arrival_grows_and_the_ends_stay(name, swap):
    case, ref = CASES[name], refined_ref(name, swap)
    for i, first, f in refined(ref):
        goal = [tuple(int(v) for v in g) for g in case["goal"][i]]
        before, after = rr.arrivals(first["path"], goal), rr.arrivals(f["path"], goal)
        assert all(y <= x for x, y in zip(before, after)), (name, i)
        assert sum(before) == f["soc_before"] and sum(after) == f["soc_after"] and max(after) == f["length"] <= first["length"]
        assert f["path"][0] == first["path"][0] == [tuple(int(v) for v in p) for p in case["pos"][i]] and f["path"][-1] == goal
        assert (f["first_status"], f["first_length"]) == (first["status"], first["length"])


@SWAP
@pytest.mark.parametrize("name", sorted(CASES))
def test_a_refinement_that_stopped_by_itself_is_a_fixed_point(name, swap):
    case, ref = CASES[name], refined_ref(name, swap)
    for i, first, f in refined(ref):
        assert f["rounds"] < rr.ROUNDS                          # every case here stops because a round adopted nothing
        again = rr.refine(ref.grid(i), f["path"], case["goal"][i], rr.ROUNDS)
        assert again["replans"] == 0 and again["rounds"] == 1 and again["path"] == f["path"]


@SWAP
def test_one_agent_walks_its_bfs_distance(swap):
    case, ref = CASES["one_agent"], refined_ref("one_agent", swap)
    d = int(er.bfs(ref.grid(0), case["goal"][0, 0])[tuple(case["pos"][0, 0])])
    assert ref.found[0]["length"] == d == 3 and ref.found[0]["soc_after"] == d


def joint_optimum(grid, start, goal):
    """The makespan optimum by breadth-first search over joint configurations; a transition is what check_transition allows: moves
    0..4 onto free cells of the frame, no two agents on one cell, no two agents exchanging cells."""
    H, W = grid.shape
    start, goal = tuple(map(tuple, start)), tuple(map(tuple, goal))
    seen, queue = {start: 0}, deque([start])
    while queue:
        Q = queue.popleft()
        if Q == goal:
            return seen[Q]
        nxt = [()]
        for a, (r, c) in enumerate(Q):
            cells = [(r + dr, c + dc) for dr, dc in er.MOVES if 0 <= r + dr < H and 0 <= c + dc < W and grid[r + dr, c + dc] == 0]
            nxt = [p + (u,) for p in nxt for u in cells if u not in p and not any(u == Q[b] and p[b] == Q[a] for b in range(a))]
        for N in nxt:
            if N not in seen:
                seen[N] = seen[Q] + 1
                queue.append(N)
    return None


def test_swap2_without_the_rule_reaches_the_joint_optimum():
    case, ref = CASES["swap2"], refined_ref("swap2")
    f = ref.found[0]
    best = joint_optimum(ref.grid(0), case["pos"][0].tolist(), case["goal"][0].tolist())
    assert (f["first_length"], f["length"], best) == (9, 6, 6)
    assert ref.metrics()[0, :5].tolist() == [1.0, 1.0, 11.0, 6.0, 6.0]


@pytest.mark.parametrize("name,first_len,length", [("grids3", 53, 15), ("offset7", 59, 19)])
def test_a_solution_over_the_cap_comes_under_it_and_is_replayed(name, first_len, length):
    case, ref = CASES[name], refined_ref(name)
    f = ref.found[0]
    assert (f["first_status"], f["first_length"], f["status"], f["length"]) == (sr.TOO_LONG, first_len, sr.SOLVED, length)
    plain = sr.run_case(case)                                   # the search alone does not replay it: its episode there is PIBT's
    assert plain.stats()[0][0] == sr.TOO_LONG and not plain.solution()[0].any() and plain.metrics()[0, 4] > length
    assert ref.metrics()[0, 0] == 1.0 and ref.metrics()[0, 4] == length and ref.solution()[0].any()
    assert np.array_equal(ref.log()[0][0, :, :length], f["solution"])


def test_with_the_rule_agents70_stays_over_the_cap_and_its_episode_is_pibts():
    case, ref = CASES["agents70"], refined_ref("agents70", True)
    f = ref.found[0]
    assert (f["first_status"], f["first_length"], f["status"], f["length"]) == (sr.TOO_LONG, 56, sr.TOO_LONG, 54) and case["steps"] == 32
    assert not ref.solution().any()
    pibt = sw.run_case(case)
    assert np.array_equal(ref.log()[0], pibt.log()[0]) and np.array_equal(ref.metrics(), pibt.metrics())


@pytest.mark.parametrize("name,inst", [("offset7", 1), ("swap2", 0)])
def test_one_round_stops_where_a_second_would_adopt_more(name, inst):
    one, full = refined_ref(name, max_rounds=1).found[inst], refined_ref(name).found[inst]
    assert one["rounds"] == 1 and 0 < one["replans"] < full["replans"] and full["rounds"] == 4
    assert full["soc_after"] < one["soc_after"] < one["soc_before"] == full["soc_before"]
    two = rr.refine(refined_ref(name).grid(inst), one["path"], CASES[name]["goal"][inst], 1)
    assert two["replans"] > 0                                   # the cap stopped it, not a round that adopted nothing


def test_a_solution_longer_than_the_horizon_is_left_alone_and_its_neighbours_are_refined():
    ref, full = refined_ref("grids3", horizon=40), refined_ref("grids3")
    f = ref.found[0]
    assert (f["status"], f["length"], f["rounds"], f["replans"], f["soc_before"], f["soc_after"]) == (sr.TOO_LONG, 53, 0, 0, 0, 0)
    assert f["solution"] is ref.first[0]["solution"] and not ref.solution()[0].any()
    for a, b in zip(ref.found[1:], full.found[1:]):
        assert a["rounds"] > 0 and a["path"] == b["path"]
    plain = sr.run_case(CASES["grids3"])
    assert np.array_equal(ref.log()[0], plain.log()[0]) and np.array_equal(ref.metrics(), plain.metrics())


@SWAP
@pytest.mark.parametrize("name,status", [("pocket", sr.EXHAUSTED), ("dead_end", sr.BUDGET)])
def test_statuses_2_and_3_are_untouched(name, status, swap):
    ref = refined_ref(name, swap)
    f = ref.found[0]
    assert (f["status"], f["first_status"], f["length"], f["rounds"], f["replans"]) == (status, status, 0, 0, 0) and f["solution"] is None
    plain = sw.run_search_case(CASES[name], swap=swap, max_iters=CASES[name]["max_iters"])
    assert np.array_equal(ref.log()[0], plain.log()[0]) and np.array_equal(ref.metrics(), plain.metrics())


@pytest.mark.parametrize("name", ["grids3", "offset7", "shared5"])
def test_refined_records_go_through_the_dataset_tokenizer(name):
    from mapf_gpt_amd import dataset_tokenizer as dt
    case, ref = CASES[name], refined_ref(name)
    keys = [{"map_name": "m", "seed": i, "num_agents": case["n_agents"]} for i in range(case["n_inst"])]
    recs = er.records(ref, keys, case["pos"], algorithm="LaCAM")
    for i, r in enumerate(recs):
        m, f = r["metrics"], ref.found[i]
        assert m["CSR"] == 1.0 and int(m["ep_length"]) == f["length"] and m["SoC"] == f["soc_after"]
        paths = dt.agent_paths(m["init_positions"], m["made_actions"])
        labels = dt.gt_actions(m["made_actions"])
        assert paths.shape == (case["n_agents"], f["length"] + 1, 2) and all(len(g) == paths.shape[1] for g in labels)
        assert np.array_equal(paths.transpose(1, 0, 2), np.asarray(f["path"]))


# what the restatement gives on the shapes of tests/test_gpu_expert_refine.py: (name, rule) -> final status, final length, first status,
# first length, SoC before, SoC after, rounds, replans per instance
PINNED = {
    ("agents65", False): ([1], [62], [1], [62], [2288], [2067], [4], [42]),
    ("agents70", False): ([3], [0], [3], [0], [0], [0], [0], [0]),
    ("dead_end", False): ([3], [0], [3], [0], [0], [0], [0], [0]),
    ("grids3", False): ([1, 1, 1], [15, 19, 9], [4, 1, 1], [53, 19, 9], [246, 73, 39], [81, 73, 39], [4, 1, 1], [11, 0, 0]),
    ("offset7", False): ([1, 1, 1], [19, 14, 13], [4, 1, 1], [59, 18, 14], [306, 105, 78], [104, 84, 77], [3, 4, 2], [7, 7, 1]),
    ("one_agent", False): ([1], [3], [1], [3], [3], [3], [1], [0]),
    ("pocket", False): ([2], [0], [2], [0], [0], [0], [0], [0]),
    ("rotation", False): ([1], [1], [1], [1], [3], [3], [1], [0]),
    ("shared5", False): ([1] * 5, [14, 15, 14, 19, 18], [1] * 5, [18, 15, 14, 19, 18], [87, 74, 87, 112, 80], [79, 72, 87, 102, 80],
                         [2, 2, 1, 2, 1], [2, 1, 0, 3, 0]),
    ("swap2", False): ([1], [6], [1], [9], [17], [11], [4], [4]),
    ("swap3", False): ([1], [12], [1], [12], [29], [29], [1], [0]),
    ("agents65", True): ([1], [50], [1], [55], [2118], [1937], [8], [46]),
    ("agents70", True): ([4], [54], [4], [56], [2397], [2250], [4], [48]),
    ("dead_end", True): ([3], [0], [3], [0], [0], [0], [0], [0]),
    ("grids3", True): ([1, 1, 1], [15, 19, 9], [4, 1, 1], [53, 19, 9], [246, 73, 39], [81, 73, 39], [4, 1, 1], [11, 0, 0]),
    ("offset7", True): ([1, 1, 1], [19, 14, 13], [1, 1, 1], [21, 18, 14], [112, 105, 78], [104, 84, 77], [2, 4, 2], [3, 7, 1]),
    ("one_agent", True): ([1], [3], [1], [3], [3], [3], [1], [0]),
    ("pocket", True): ([2], [0], [2], [0], [0], [0], [0], [0]),
    ("rotation", True): ([1], [1], [1], [1], [3], [3], [1], [0]),
    ("shared5", True): ([1] * 5, [14, 15, 14, 19, 18], [1] * 5, [16, 15, 14, 19, 18], [85, 74, 87, 112, 80], [79, 72, 87, 102, 80],
                        [2, 2, 1, 2, 1], [2, 1, 0, 3, 0]),
    ("swap2", True): ([1], [6], [1], [6], [11], [11], [1], [0]),
    ("swap3", True): ([1], [29], [1], [29], [84], [84], [1], [0]),
}


@SWAP
def test_statistics_of_the_gpu_shapes(swap):
    for name in sorted(CASES):
        ref = refined_ref(name, swap)
        st = ref.stats()
        got = tuple(x.tolist() for x in (st[0], st[3]) + ref.refine_stats())
        if name == "empty32":                                   # 32 instances: all solved at once; two of them gain a step of SoC or length
            assert got[0] == got[2] == [1] * 32 and sum(got[6]) == 34 and sum(got[7]) == 2
            assert sum(got[3]) - sum(got[1]) == 2 and sum(got[4]) - sum(got[5]) == 6
        else:
            assert got == PINNED[name, swap], (name, swap, got)
