"""The corridor swap rule's spec on the host (tests/expert_swap_ref.py): the invariants of section 20 on every
transition of every case, with the restatement's env landing every agent on its planned cell; the corridor swaps the rule solves; a
hand case for every branch of the rule; the walk cap; and the restatement's counts on the dataset's maze."""
import numpy as np
import pytest

from tests import expert_ref as er
from tests import expert_search_ref as sr
from tests import expert_swap_ref as sw
from tests.test_expert_cpu import check_step, digest

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


# digests (tests/test_expert_cpu.py: digest, and where they come from): name -> (PIBT with the rule, the search with the rule in front)
DIGESTS = {
    "agents65": ("792e8eebc919acae88410c781831981468d8a13e29c540ebe1bdda2e4aebaca0",
        "0a0baf20e847060d44e35a5e4a8d08d1479ce3ec8c95123bf5040cd8c12ace0b"),
    "agents70": ("be1fce2b6b4810fa59c396ac19aa80a010b8654a3bd7be3a2afcd064565a6f64",
        "ceb9981309a4b72ddeda722460f4099cd430f750f960b03c12490cca3369e5a7"),
    "clear2": ("ba89fc421df34d420fcdc81d6bd5e0c9ddcd8a8d11a49cd4f1f957ac718c3292",
        "b6ffdbea12a861fff8ff02f93d5d63b448f26f63a956cabe7a5625d1aa6ec4ef"),
    "dead_end": ("e4ad371d0863106482f2143dae3b48cde24b77ecf7dc2603733460c285541c18",
        "773880d9c66bb4dcc9c5d220ef71cc8b2d994ca57d0a2c0c45547041133f8a4a"),
    "grids3": ("8f64937b328f17de5243f9c3d2a2ae67eb895e7d626f60374aed30768f2c5012",
        "041241b1d0d09896505035209183766bafbbca667b1885f25ccf4e6903ef2237"),
    "maze16": ("709adb895e7fdb8421d1d06c8b7d0d443fea7054219766ddae1bfe2c66bdc7e5",
        "dee6eec1bea3d6513c8cf0c0d4f137743eb1eea250a42112ba0bbf152609af9a"),
    "offset7": ("2629b015d99ef419fd4b70ad550a2ac8f264ec549bd5fde64a4a953ceee4e8ae",
        "681a7c560904fd09ab6e9638e889886ae3c591d74ca3c6092a3879a10600ec1d"),
    "one_agent": ("8ea4d162561388b8d808b7ba214d0dd26f03ca388f1d03f047eb30c273cbdcf9",
        "88d1f05a50ef80492dc0e61bc8f8fc1983762bd3a920b20df77c276c7e03a4cb"),
    "own3": ("c85aaf7cf0bdfdca1157b633d113da9e79d76f91be8d63613f3b752ee27662db",
        "02614ce073c42b0cfdedff9c8b893ca5994adc9e40fc204fff5b9125c9db548c"),
    "pocket": ("74f400dd2d16e04fc3349ec6ad42f63404151396d68388ba1639d7315038c22f",
        "6edf3eb6adf4b5d4c45550738f0658b1421bc2eb20989f4b089efb713c289e37"),
    "reserved4": ("fa8b0831bd96e9a5896ea2979fe94a1106ae87ff0896be69c6eb8a8ed161b11b",
        "056445694760538efdae481703f22fdefa133b72321d2e19d74a060b1e21b2b1"),
    "rests3": ("19f9fb4659300c36f8bce098eba71e2ff10fafafdb01e51c30d1f6352a0b4c93",
        "ec10595cf544cd6143c4612d93b536cc237064c8ef835b177b1f51158cc38596"),
    "ring2": ("d88cbaa5b86b2a1777a041380e785a170e70bc6cfccd155c48449a8e1adeaaf5",
        "ef1ae677f109072571664aadec2a89e28e0d15f45a1a34d600180231442e26b3"),
    "rotation": ("4d169063e2b52792a2e1bf65a51733510d2951d58bdae06e2612182b9d9159d5",
        "1b5b8b9ce97303ce362817d284db3f2dbb3af037c70e311c66168b14339f28d4"),
    "shared5": ("d8ddc0b589403aed654f9760417d5fb29cd9cda167955abac4f6a6ff0725ddee",
        "d8ab34e3507730b3d99c5f282af871f49d7d4d402234a62ed0ef06172056f525"),
    "swap2": ("407323cd545b7c4e6c983ffb2552bba9a1c8c771945dc4c7578da1611f1d7f1e",
        "c18b185f0c84ae2eb4e050320457dffc6e738facdec3391f96d5a39747170409"),
    "swap3": ("cce206207e1d2c8264ba62fa3e5921f5e5df967a9ac46806eda94bcc2edcbeac",
        "51947f40e92014356ffa61f9915c1edf7252a03de7b033d49889aa532b69bcfc"),
}


def test_the_episodes_and_searches_are_bit_for_bit_what_they_were():
    assert set(CASES) == set(DIGESTS)
    assert {name: (digest(episode(name)), digest(searched(name))) for name in sorted(CASES)} == DIGESTS
