"""The collision shield on lifelong episodes on the host.  No device.

The episode tests run the restatement alone (tests/shield_lifelong_ref.py: the lifelong restatement with the shield's plan, composed, no
loop of its own) on the shapes tests/test_gpu_shield_lifelong.py compares the device against, with the same seeded logits: they pass on
the parent commit too and say nothing about the kernel.  What they are for: the invariants of every step by the independent checker, the
three properties of section 31 with respect to the fields of the goals held now, the arrival count, and the conditions that keep the
device tests from passing vacuously (arrivals, overrides, wrapped queues).  The last tests need the feature: the binding of
mgpt_expert_set_shield_lifelong and the new keywords of BatchedExpert, BatchedRunner and MAPFGPTInferenceConfig."""
import inspect

import numpy as np
import pytest

from tests import expert_checks as ck
from tests import expert_ref as er
from tests import shield_lifelong_ref as slr
from tests import shield_ref as sr

CASES = slr.cases()
_runs = {}


def run(name):
    """The finished restatement of a shape (run once, with every step checked), and the count of steps that met property 2's premise."""
    if name in _runs:
        return _runs[name]
    case = CASES[name]
    n_inst = case["n_inst"]
    ref = slr.new_ref(case)
    rng = np.random.default_rng(slr.SEED)
    none = np.zeros(n_inst, bool)
    fed_back = kept = 0
    for t in range(case["steps"]):
        bits, first = slr.step_inputs(ref, rng, t)
        before, held, since, over = ref.pos.copy(), ref.goal.copy(), ref.since.copy(), ref.overrides.copy()
        dist = [[d.copy() for d in ref.dist[i]] for i in range(n_inst)]                    # the fields the plan read: of the goals held now
        free = [sr.is_collision_free(ref.grid(i), before[i], dist[i], first[i]) for i in range(n_inst)]
        actions, planned = ref.step(bits, first)
        # 1. section 20's invariants, and the env (default rules) leaves every agent on its planned cell
        ck.check_transition(case["grids"], before, actions, planned, ref.pos, none)
        for i in range(n_inst):
            if free[i]:                                  # 2. a collision-free joint action comes back unchanged
                fed_back += 1
                assert np.array_equal(actions[i], first[i]) and ref.overrides[i] == over[i]
            else:
                assert ref.overrides[i] == over[i] + int((actions[i] != first[i]).sum())
            kept += property_3(ref.grid(i), before[i], dist[i], since[i], first[i], actions[i])
        on = (ref.pos == held).all(-1)                   # section 30's rules: against the goal held during the step
        assert [ref.arrivals[i][t] for i in range(n_inst)] == on.sum(1).tolist()
        assert (ref.since[on] == 0).all() and np.array_equal(ref.since[~on], since[~on] + 1)
        assert np.array_equal(ref.arrivals_log().sum(1), ref.reached.sum(1))
    assert (ref.done == 2).all()                         # truncation only
    assert kept > 0
    _runs[name] = (ref, fed_back)
    return _runs[name]


def property_3(grid, pos, dist, since, first, actions):
    """Section 31's property 3 as section 20's PIBT gives it ("property 3"): the agent first in the order plans
    with nothing reserved and no parent, so if its `first` is a candidate it keeps it -- unless another agent stands on that cell and
    cannot give way (the inheritance fails, as in a dead end); that agent then stays where it is and the first agent goes on to its next
    candidate.  -> 1 if the first agent's `first` was a candidate and it kept it."""
    a = er.priority_order(since)[0]
    k = int(first[a])
    if k not in sr.candidate_actions(grid, pos, dist, a):
        return 0
    if actions[a] == k:
        return 1
    u = (int(pos[a][0]) + er.MOVES[k][0], int(pos[a][1]) + er.MOVES[k][1])
    on_u = [c for c in range(len(pos)) if c != a and (int(pos[c][0]), int(pos[c][1])) == u]
    assert len(on_u) == 1 and actions[on_u[0]] == 0, "the first agent in the order lost a free first candidate"
    return 0


def test_the_shapes_are_the_non_swap_shapes_of_the_lifelong_expert():
    assert sorted(CASES) == ["agents65", "agents70", "duplicates", "grids3", "offset7", "one_agent", "own_cell", "pocket", "same_goal2",
                             "shared5", "wrap1"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_step_keeps_the_invariants_the_three_properties_and_the_arrival_count(name):
    ref, fed_back = run(name)
    assert fed_back > 0 or CASES[name]["n_agents"] >= 65      # (65 agents on 16 x 16 never sample a collision-free joint action)
    assert np.array_equal(ref.arrivals_log().sum(1), ref.reached.sum(1))
    assert ref.throughput().tolist() == (ref.reached.sum(1).astype(np.float32) / np.float32(CASES[name]["steps"])).tolist()


def test_the_device_tests_cannot_pass_vacuously():
    """On the restatement alone: every instance arrives, every instance of 8 or more agents is overridden, and in at least two shapes an
    agent has more arrivals than its queue has entries (the wrap)."""
    wrapped = []
    for name in sorted(CASES):
        ref, _ = run(name)
        assert (ref.reached.sum(1) >= 1).all(), name
        if CASES[name]["n_agents"] >= 8:
            assert (ref.overrides >= 1).all(), name
        if (ref.reached > CASES[name]["queue"].shape[2]).any():
            wrapped.append(name)
    assert len(wrapped) >= 2, wrapped


# what the restatement gives with SEED: name -> (arrivals per instance, overrides per instance)
OUTCOMES = {
    "agents65": ([61], [1125]),
    "agents70": ([80], [1252]),
    "duplicates": ([5], [0]),
    "grids3": ([16, 24, 19], [50, 26, 24]),
    "offset7": ([10, 16, 18], [39, 82, 38]),
    "one_agent": ([7], [4]),
    "own_cell": ([4], [1]),
    "pocket": ([2], [18]),
    "same_goal2": ([5], [3]),
    "shared5": ([17, 16, 11, 18, 9], [34, 54, 64, 37, 89]),
    "wrap1": ([3], [3]),
}


def test_the_outcomes_of_the_shapes_are_pinned():
    got = {name: (run(name)[0].reached.sum(1).tolist(), run(name)[0].overrides.tolist()) for name in CASES}
    assert got == OUTCOMES


def test_a_next_goal_on_the_agents_own_cell_and_duplicate_entries_count_on_the_wait():
    """Section 30's two consequences, with a policy that walks straight to the goal (first = the best action, no noise): the agent of
    own_cell arrives, finds its next goal under its feet and arrives again on the following step's wait; the agent of duplicates arrives
    at queue[0] and, queue[1] being the same cell, again one step later."""
    for name, want in (("own_cell", [0, 1, 1]), ("duplicates", None)):
        case = CASES[name]
        ref = slr.new_ref(case)
        for t in range(case["steps"]):
            bits, _ = slr.goal_seeking_logits(ref, _NoNoise())
            first = bits.view(np.float32)[..., :5].argmax(-1)
            actions, _ = ref.step(bits, first)
            assert np.array_equal(actions, first) and ref.overrides[0] == 0               # one agent: nothing to resolve
        if want is not None:
            assert ref.arrivals[0][:3] == want and ref.made[0][0][2] == 0
        else:
            steps = [t for t, n in enumerate(ref.arrivals[0]) if n]
            assert steps[2] == steps[1] + 1 and ref.made[0][0][steps[2]] == 0
        assert sum(ref.arrivals[0]) == ref.reached[0, 0]


class _NoNoise:
    """A generator whose integers are 0 and whose uniforms are 0: goal_seeking_logits without noise, `first` = the argmax."""

    def integers(self, lo, hi, size):
        return np.zeros(size, np.int64)

    def random(self, size):
        return np.zeros(size)


# ---- what needs the feature (fails on the parent commit) -------------------------------------------------------------------------------
def test_the_library_binds_the_setter():
    from mapf_gpt_amd import _lib, build
    build.build()
    assert _lib.SYMBOLS["mgpt_expert_set_shield_lifelong"][1] == [_lib._vp, _lib._i]
    L = _lib.lib()
    assert hasattr(L, "mgpt_expert_set_shield_lifelong")
    assert L.mgpt_expert_set_shield_lifelong(None, 1) == _lib.ERR_ARG and b"NULL" in L.mgpt_last_error()


def test_the_new_keywords_exist_and_default_to_off():
    from mapf_gpt_amd.expert import BatchedExpert
    from mapf_gpt_amd.inference import MAPFGPTInferenceConfig
    from mapf_gpt_amd.runner import BatchedRunner
    for cls in (BatchedExpert, BatchedRunner):
        assert inspect.signature(cls.__init__).parameters["shield_lifelong"].default is False
    assert MAPFGPTInferenceConfig().shield_lifelong is False
    assert MAPFGPTInferenceConfig(shield="pibt", shield_lifelong=True).shield_lifelong is True


def test_argument_errors_that_need_no_device():
    from mapf_gpt_amd import expert, runner
    grid = np.zeros((12, 12), np.uint8)
    with pytest.raises(ValueError, match="shield_lifelong"):
        expert.BatchedExpert(grid, 1, 2, 8, shield_lifelong=True)
    with pytest.raises(ValueError, match="shield_lifelong"):
        runner.BatchedRunner(grid, 1, 2, None, shield_lifelong=True)
    ex = expert.BatchedExpert.__new__(expert.BatchedExpert)                                 # reset()'s own checks come before any device call
    ex.lifelong, ex.shield, ex.shield_lifelong, ex.n_inst, ex.n_agents, ex._h = False, True, True, 2, 3, None
    with pytest.raises(ValueError, match="shield_lifelong=True.*goal_queue"):
        ex.reset(None, None)
    with pytest.raises(ValueError, match="goal_queue"):
        ex.reset(None, None, goal_queue=np.zeros((2, 4, 4, 2), np.int16))
    ex.shield_lifelong = False
    with pytest.raises(ValueError, match="lifelong=True"):
        ex.reset(None, None, goal_queue=np.zeros((2, 3, 4, 2), np.int16))
    run = runner.BatchedRunner.__new__(runner.BatchedRunner)
    run.shield_lifelong, run._step = True, None
    with pytest.raises(ValueError, match="goal_queue"):
        run.reset(None, None)
    run.shield_lifelong = False
    with pytest.raises(RuntimeError, match="shield_lifelong"):
        run.arrivals()
