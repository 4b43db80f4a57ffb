"""The collision shield's restatement (tests/shield_ref.py) alone: the three properties of DESIGN.md section 31 on every step of random
episodes, checked by the independent checker (tests/expert_checks.py) and the env restatement; the preference order on hand-written
bit patterns; a head-on pair in a corridor; a three-agent rotation.  No device."""
import numpy as np
import pytest

from tests import expert_checks as ck
from tests import expert_ref as er
from tests import shield_ref as sr

EPISODES = {
    "agents8": er.random_case(12, 12, 0.2, 2, 8, 24, seed=0),
    "crowded": er.random_case(8, 8, 0.1, 1, 24, 16, seed=0, map_seed=5),
}


@pytest.mark.parametrize("name", sorted(EPISODES))
def test_the_three_properties_on_every_step_of_random_episodes(name):
    case = EPISODES[name]
    n_inst, n = case["n_inst"], case["n_agents"]
    ref = sr.RefShield(case["grids"], n_inst, n, case["steps"])
    ref.reset(case["pos"], case["goal"])
    rng = np.random.default_rng(17)
    fed_back = 0
    for t in range(case["steps"]):
        bits = sr.random_logits(rng, n_inst, n)
        first = rng.integers(0, 5, size=(n_inst, n))
        if t % 3 == 2:                                   # property 2's premise: a collision-free joint action, from another plan
            for i in range(n_inst):
                first[i] = sr.plan(ref.grid(i), ref.pos[i], ref.dist[i], ref.since[i], first[i], sr.random_logits(rng, 1, n)[0])[1]
        before, since, skip, over = ref.pos.copy(), ref.since.copy(), ref.done.copy() != 0, ref.overrides.copy()
        free = [not skip[i] and sr.is_collision_free(ref.grid(i), before[i], ref.dist[i], first[i]) for i in range(n_inst)]
        actions, planned = ref.step(bits, first)
        # 1. section 20's invariants, and the env (default rules) leaves every agent on its planned cell
        ck.check_transition(case["grids"], before, np.where(skip[:, None], 0, actions), planned, ref.pos, skip)
        for i in range(n_inst):
            if skip[i]:
                continue
            if free[i]:                                  # 2. a collision-free joint action comes back unchanged
                fed_back += 1
                assert np.array_equal(actions[i], first[i]) and ref.overrides[i] == over[i]
            else:
                assert ref.overrides[i] == over[i] + int((actions[i] != first[i]).sum())
            for a in er.priority_order(since[i]):       # 3. the first agent in the order whose `first` is a candidate keeps it
                if int(first[i, a]) in sr.candidate_actions(ref.grid(i), before[i], ref.dist[i], a):
                    assert actions[i, a] == first[i, a]
                    break
    assert fed_back >= case["steps"] // 3


@pytest.mark.parametrize("name", sorted(sr.hand_patterns()))
def test_preference_order_on_hand_written_bit_patterns(name):
    bits, first, cand, want = sr.hand_patterns()[name]
    assert sr.preference(cand, first, bits) == want


def test_the_monotone_map_is_a_total_order_on_bit_patterns():
    ordered = [sr.NEG_QNAN, sr.NEG_INF, sr.MINUS_ONE, sr.NEG_ZERO, sr.POS_ZERO, sr.ONE, sr.TWO, sr.POS_INF, sr.QNAN]
    keys = [sr.monotone(b) for b in ordered]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert sr.monotone(sr.bits_of(np.float32(-0.0))[0]) < sr.monotone(sr.bits_of(np.float32(0.0))[0])
    vals = np.array([-3.5, -1.0, -1e-30, 1e-30, 0.25, 7.0], np.float32)       # on ordinary values it is the order of the floats
    assert [sr.monotone(b) for b in sr.bits_of(vals)] == sorted(sr.monotone(b) for b in sr.bits_of(vals))


def _one(grid_rows, pos, goal):
    grids, pos, goal = er._parse(grid_rows), er._cells(pos), er._cells(goal)
    ref = sr.RefShield(grids, 1, pos.shape[1], 8)
    ref.reset(pos, goal)
    return grids, ref


def test_a_head_on_pair_in_a_corridor_does_not_swap():
    grids, ref = _one(["#######", "#.....#", "#######"], [(1, 2), (1, 3)], [(1, 5), (1, 1)])
    before = ref.pos.copy()
    first = np.array([[4, 3]])                           # right and left: into each other
    bits = np.tile(np.array([sr.MINUS_ONE, sr.MINUS_ONE, sr.MINUS_ONE, sr.ONE, sr.TWO], np.uint32), (1, 2, 1))
    actions, planned = ref.step(bits, first)
    ck.check_transition(grids, before, actions, planned, ref.pos, np.zeros(1, bool))
    assert actions[0, 0] == 4                            # property 3: agent 0 is first in the order
    assert actions[0, 1] in (0, 4) and actions[0, 1] != 3      # agent 1 waits or backs out; here it is pushed right
    assert actions[0].tolist() == [4, 4] and ref.overrides[0] == 1


def test_a_three_agent_rotation_is_returned_unchanged():
    case = er.hand_cases()["rotation"]                   # 2 x 2 block, three agents, each wanting the cell of the next
    ref = sr.RefShield(case["grids"], 1, 3, 4)
    ref.reset(case["pos"], case["goal"])
    before = ref.pos.copy()
    first = np.array([[4, 2, 3]])                        # (1,1) -> (1,2) -> (2,2) -> (2,1)
    assert sr.is_collision_free(ref.grid(0), before[0], ref.dist[0], first[0])
    bits = np.tile(np.array([sr.TWO, sr.ONE, sr.ONE, sr.ONE, sr.ONE], np.uint32), (1, 3, 1))      # the logits prefer waiting
    actions, planned = ref.step(bits, first)
    ck.check_transition(case["grids"], before, actions, planned, ref.pos, np.zeros(1, bool))
    assert actions[0].tolist() == [4, 2, 3] and ref.overrides[0] == 0
