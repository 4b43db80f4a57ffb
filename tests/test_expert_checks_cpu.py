"""The independent checker (tests/expert_checks.py) on the host: it accepts every step the three restatements produce on their GPU
shapes and its replay reproduces their final cells and metrics; it rejects one hand-made violation per assertion.  Without the second
part the device tests that rest on it (tests/test_gpu_expert_scale.py) could pass vacuously."""
import numpy as np
import pytest

from tests import expert_checks as ck
from tests import expert_ref as er
from tests import expert_search_ref as sr
from tests import expert_swap_ref as sw

RUNS = [(f"{kind}-{name}", kind, name) for kind, cases in (("pibt", er.gpu_cases()), ("search", sr.gpu_cases()), ("swap", sw.gpu_cases()),
                                                          ("swap_search", sw.gpu_cases())) for name in sorted(cases)]
START = {"pibt": (er.gpu_cases, er.run_case), "search": (sr.gpu_cases, sr.run_case), "swap": (sw.gpu_cases, sw.run_case),
         "swap_search": (sw.gpu_cases, sw.run_search_case)}


@pytest.mark.parametrize("kind,name", [r[1:] for r in RUNS], ids=[r[0] for r in RUNS])
def test_checker_and_replay_accept_the_restatements_own_output(kind, name):
    cases, run = START[kind]
    case = cases()[name]
    ref = run(case, steps=0)
    pos0 = ref.pos.copy()
    for t in range(case["steps"]):
        before, skip = ref.pos.copy(), ref.done != 0
        act, planned = ref.step()
        ck.check_transition(case["grids"], before, act, planned, ref.pos, skip)
    log, lens = ref.log()
    final, metrics = ck.replay(case["grids"], pos0, ref.goal, log, lens)
    assert np.array_equal(final, ref.pos)
    assert np.array_equal(metrics, ref.metrics()[:, :5]), (metrics, ref.metrics()[:, :5])
    assert np.array_equal(metrics[:, 4], lens)


def valid_step():
    """One valid step of two instances of four agents on a 5 x 5 room with a wall at (2, 2) (no border: the frame itself bounds it).
    Instance 0: agent 0 moves right into a free cell, agent 1 follows it, agent 2 moves down, agent 3 waits.  Instance 1 is done."""
    grid = np.zeros((1, 5, 5), np.uint8)
    grid[0, 2, 2] = 1
    pos = np.array([[(0, 1), (0, 0), (3, 4), (4, 0)]] * 2, np.int16)
    actions = np.array([[4, 4, 2, 0], [0, 0, 0, 0]], np.int32)
    planned = np.array([[(0, 2), (0, 1), (4, 4), (4, 0)], [(0, 1), (0, 0), (3, 4), (4, 0)]], np.int16)
    return dict(grids=grid, pos=pos, actions=actions, planned=planned, pos_after=planned.copy(), skip=np.array([False, True]))


def test_the_valid_step_passes():
    ck.check_transition(**valid_step())


# one entry of the valid step edited per violation: what the message names -> (array, index, new value).  An edited planned cell also
# leaves its action and pos_after behind; the checker reports the invariants of the plan itself first
VIOLATIONS = {
    "vertex conflict": ("planned", (0, 3), (4, 4)),             # agent 3 plans agent 2's next cell
    "edge swap": ("planned", (0, 0), (0, 0)),                   # agent 0 plans agent 1's cell while agent 1 plans agent 0's
    "blocked cell": ("planned", (0, 2), (2, 2)),                # agent 2 plans the wall
    "does not match the move": ("actions", (0, 2), 1),          # agent 2 moved down, its action says up
    "pos_after": ("pos_after", (0, 0), (0, 1)),                 # the env left agent 0 where it was
}


@pytest.mark.parametrize("what", sorted(VIOLATIONS))
def test_the_checker_rejects_one_violation_per_assertion(what):
    step = valid_step()
    field, index, value = VIOLATIONS[what]
    step[field][index] = value
    with pytest.raises(AssertionError, match=what):
        ck.check_transition(**step)


def test_the_checker_rejects_a_done_instance_that_acts_and_a_cell_outside_the_frame():
    step = valid_step()
    step["actions"][1, 0] = 4
    with pytest.raises(AssertionError, match="skipped"):
        ck.check_transition(**step)
    step = valid_step()
    step["planned"][1, 2] = (4, 4)
    with pytest.raises(AssertionError, match="skipped"):
        ck.check_transition(**step)
    step = valid_step()
    step["pos"][0, 2], step["actions"][0, 2], step["planned"][0, 2], step["pos_after"][0, 2] = (4, 4), 2, (5, 4), (5, 4)
    with pytest.raises(AssertionError, match="outside the frame"):
        ck.check_transition(**step)


def test_trajectory_metrics_by_hand():
    goal = np.array([(0, 2), (1, 1)])
    # agent 0 reaches its goal at step 2, leaves it at 3 and is back at 4; agent 1 arrives at 3 and stays: the episode ends at step 4
    traj = np.array([[(0, 0), (1, 0)], [(0, 1), (1, 0)], [(0, 2), (1, 0)], [(0, 1), (1, 1)], [(0, 2), (1, 1)], [(0, 2), (1, 1)]])
    assert ck.trajectory_metrics(traj, goal).tolist() == [1.0, 1.0, 7.0, 4.0, 4.0]              # the step after the end is not counted
    assert ck.trajectory_metrics(traj[:4], goal).tolist() == [0.0, 0.5, 6.0, 3.0, 3.0]          # cut short: agent 0 is off its goal
    assert ck.trajectory_metrics(traj[:3], goal).tolist() == [0.0, 0.5, 4.0, 2.0, 2.0]
    assert ck.trajectory_metrics(traj[4:], goal).tolist() == [1.0, 1.0, 0.0, 0.0, 1.0]          # all on their goals at reset: one step
