"""The corridor swap rule's spec on the host (tests/expert_swap_ref.py): the invariants of section 20 on every
transition of every case, with the restatement's env landing every agent on its planned cell; the corridor swaps the rule solves; a
hand case for every branch of the rule; the walk cap; and the restatement's counts on the dataset's maze."""
import numpy as np
import pytest

from tests import expert_ref as er
from tests import expert_search_ref as sr
from tests import expert_swap_ref as sw
from tests.test_expert_cpu import check_step

CASES = sw.gpu_cases()
HAND = sorted(sw.hand_cases())
_EPISODES, _SEARCHES = {}, {}


def episode(name):
    """PIBT with the rule over the case's whole episode, every step checked (computed once, read only)."""
    if name not in _EPISODES:
        _EPISODES[name] = checked_episode(CASES[name])
    return _EPISODES[name]


def searched(name):
    if name not in _SEARCHES:
        _SEARCHES[name] = sw.run_search_case(CASES[name])
    return _SEARCHES[name]


def checked_episode(case, cap=None):
    ref = sw.run_case(case, steps=0, cap=cap)
    n = case["n_agents"]
    for _ in range(case["steps"]):
        for i in range(case["n_inst"]):
            if ref.done[i]:
                continue
            nxt, act, _ = sw.plan(ref.grid(i), ref.pos[i], ref.dist[i], ref.since[i], ref.seed, ref.t, (case["inst_offset"] + i) * n,
                                  True, cap)
            check_step(ref.grid(i), ref.pos[i], nxt, act)           # distinct, no swap, no blocked cell, one cell; the oracle's env
        _, planned = ref.step()
        assert np.array_equal(ref.pos, planned), "the restatement's env left an agent off its planned cell"
    return ref


def check_solution(case, ref):
    for i, f in enumerate(ref.found):
        if f["status"] not in (sr.SOLVED, sr.TOO_LONG):
            continue
        grid, path = ref.grid(i), f["path"]
        assert path[0] == [tuple(int(v) for v in p) for p in case["pos"][i]]
        assert path[-1] == [tuple(int(v) for v in g) for g in case["goal"][i]]
        for t in range(f["length"]):
            act = f["solution"][:, t].tolist()
            check_step(grid, path[t], path[t + 1], act)
            assert er.env_step(grid, path[t], act) == path[t + 1]


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_step_of_an_episode_keeps_the_invariants(name):
    episode(name)


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_transition_of_a_solution_keeps_the_invariants(name):
    check_solution(CASES[name], searched(name))


def test_with_the_switch_off_the_restatement_is_the_existing_one():
    for name in ("swap3", "shared5", "pocket"):
        case = CASES[name]
        a, b = sw.run_case(case, swap=False), er.run_case(case)
        assert np.array_equal(a.log()[0], b.log()[0]) and np.array_equal(a.metrics(), b.metrics()) and a.trace == {}
        s, r = sw.run_search_case(case, swap=False), sr.run_case(case, max_iters=sw.MAX_ITERS)
        assert [x.tolist() for x in s.stats()] == [x.tolist() for x in r.stats()] and np.array_equal(s.log()[0], r.log()[0])


def test_pibt_with_the_rule_solves_swap2_in_six_steps():
    case = CASES["swap2"]
    assert er.run_case(dict(case, steps=64)).metrics()[0, 0] == 0.0      # unsolved in 64 steps without the rule
    m = episode("swap2").metrics()[0]
    assert m[0] == 1.0 and m[4] == 6
    assert episode("swap2").trace == {"swap": 1, "pull": 1}


# the search with the rule, max_iters 256: name -> (status, iterations, nodes, length) per instance
PINNED = {
    "swap2": ([1], [7], [7], [6]),
    "swap3": ([1], [95], [30], [29]),
    "pocket": ([2], [62], [6], [0]),
    "rotation": ([1], [2], [2], [1]),
    "dead_end": ([3], [256], [1], [0]),
    "clear2": ([1], [5], [5], [4]),
    "rests3": ([4], [155], [27], [25]),
    "ring2": ([1], [20], [9], [8]),
    "own3": ([4], [38], [22], [21]),
    "reserved4": ([3], [256], [5], [0]),
    "one_agent": ([1], [4], [4], [3]),
    "agents65": ([4], [56], [56], [55]),
    "agents70": ([4], [57], [57], [56]),
    "grids3": ([4, 1, 1], [113, 20, 10], [54, 20, 10], [53, 19, 9]),
    "shared5": ([1, 1, 1, 1, 1], [17, 16, 15, 20, 19], [17, 16, 15, 20, 19], [16, 15, 14, 19, 18]),
    "offset7": ([1, 1, 1], [22, 19, 15], [22, 19, 15], [21, 18, 14]),
    "maze16": ([1, 1, 1, 1], [85, 201, 57, 78], [85, 122, 57, 78], [84, 121, 56, 77]),
}
# solved episodes (CSR = 1): name -> (PIBT with the rule, the search with the rule in front)
SOLVED = {"swap2": (1, 1), "swap3": (0, 1), "pocket": (0, 0), "rotation": (1, 1), "dead_end": (0, 0), "clear2": (1, 1), "rests3": (0, 0),
          "ring2": (0, 1), "own3": (0, 0), "reserved4": (0, 0), "one_agent": (1, 1), "agents65": (0, 0), "agents70": (0, 0), "grids3": (3, 3),
          "shared5": (5, 5), "offset7": (3, 3), "maze16": (4, 4)}


def test_status_iteration_node_and_solved_counts():
    """Values of the restatement (the device must equal it case by case; no share of solved episodes is a bar anywhere).  swap2 and
    swap3 under the search: 7 iterations / 6 steps and 95 / 29.  The maze at 16 agents x 4 instances: PIBT alone solves 1 of 4."""
    assert set(PINNED) == set(CASES) == set(SOLVED)
    for name in sorted(CASES):
        assert tuple(s.tolist() for s in searched(name).stats()) == PINNED[name], name
        got = (int(episode(name).metrics()[:, 0].sum()), int(searched(name).metrics()[:, 0].sum()))
        assert got == SOLVED[name], (name, got)
    assert int(er.run_case(CASES["maze16"]).metrics()[:, 0].sum()) == 1


def test_the_old_hand_cases_come_out_as_before_or_better():
    for name in ("dead_end", "rotation", "pocket"):             # as they come out: the rule finds nothing to swap in them
        a, b = episode(name), er.run_case(CASES[name])
        assert np.array_equal(a.log()[0], b.log()[0]) and np.array_equal(a.metrics(), b.metrics()), name
    assert searched("pocket").stats()[0].tolist() == [sr.EXHAUSTED]


@pytest.mark.parametrize("name", sorted(sw.BRANCH))
def test_a_hand_case_reaches_its_branch(name):
    branch, step = sw.BRANCH[name]
    ref = sw.run_case(CASES[name], steps=step)
    assert branch not in ref.trace
    ref.step()
    assert ref.trace.get(branch, 0) >= 1, ref.trace


def test_the_clear_branch_moves_the_agent_away_for_its_neighbours_swap():
    ref = sw.run_case(CASES["clear2"], steps=1)                  # agents on (1,2) and (1,3) of #.....# with the pocket under (1,3)
    act, _ = ref.step()
    assert ref.trace == {"clear": 1} and act[0].tolist() == [4, 2]       # agent 1 steps down into the pocket, agent 0 passes
    assert episode("clear2").metrics()[0, 0] == 1.0


def test_an_own_cell_first_or_a_reserved_cell_refuse_the_pull():
    ref = sw.run_case(CASES["own3"], steps=0)
    act, planned = ref.step()
    assert ref.trace == {"swap": 1, "pull_own": 1} and act[0].tolist() == [0, 0, 0]
    ref = sw.run_case(CASES["reserved4"], steps=0)
    act, planned = ref.step()
    assert ref.trace == {"swap": 1, "pull_reserved": 1}
    assert act[0].tolist() == [4, 4, 0, 4]                      # agent 2, the swap agent, is not pulled: it stays in the stub


@pytest.mark.parametrize("name", HAND)
def test_with_the_walk_cap_at_one_the_invariants_hold(name):
    ref = checked_episode(CASES[name], cap=1)
    check_solution(CASES[name], sw.run_search_case(CASES[name], cap=1))
    if name in ("swap2", "swap3"):
        assert ref.trace.get("cap", 0) >= 1                     # the corridor is longer than one advance: the cap is what ends the walk


def test_the_cap_does_not_bind_on_the_test_shapes():
    for name in sorted(CASES):
        assert "cap" not in episode(name).trace and "cap" not in searched(name).trace, name
