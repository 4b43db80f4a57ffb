"""The expert's lifelong mode at the shapes of the evaluation sets, checked without a restatement of the planner:

    wfi_warehouse, 16 instances x 192 agents, 48 steps: plain PIBT
    validation-mazes-seed-000, 64 instances x 32 agents, 64 steps: PIBT with the swap rule

After every step check_transition (tests/expert_checks.py) holds on the device's own output, and the arrivals the expert logged for the
step are the agents whose new cell is the goal read back before the step.  At the end targets() walked by dataset_tokenizer.goal_positions
along the logged paths reproduces the goal read back after every step, and every instance has arrivals: starts, goals and queues lie in
one component, so an instance without one in 48 steps and more would be the planner's fault (the restatement on two instances of each
shape, on the host: 151 and 157 arrivals in the warehouse instances, 86 and 87 in the maze's)."""
import numpy as np
import pytest

from tests import expert_checks as ck
from tests.expert_lifelong_ref import _no_agent_starts_on_its_goal
from tests.expert_shapes import named_case

pytestmark = pytest.mark.gpu
QUEUE = 16
SHAPES = {"warehouse": dict(name="wfi_warehouse", n_inst=16, n_agents=192, steps=48, seed=6, swap=False),
          "maze": dict(name="validation-mazes-seed-000", n_inst=64, n_agents=32, steps=64, seed=5, swap=True)}


def case_of(shape, n_inst=None):
    """named_case with the queue evaluation.py would seed for run 100 + i, no agent starting on its own goal."""
    from mapf_gpt_amd import evaluation as ev, maps
    s = dict(SHAPES[shape])
    swap = s.pop("swap")
    s["n_inst"] = n_inst or s["n_inst"]
    case = named_case(max_iters=0, **s)
    frame = maps.load_named(s["name"])
    case.update(swap=swap, queue=np.stack([ev.lifelong_queue(frame, 100 + i, s["n_agents"], QUEUE) for i in range(s["n_inst"])]))
    return _no_agent_starts_on_its_goal(case)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_step_is_a_valid_transition_and_the_arrivals_are_the_envs(shape):
    import torch
    from mapf_gpt_amd import dataset_tokenizer as dt
    from mapf_gpt_amd.expert import BatchedExpert
    case = case_of(shape)
    n_inst, n, T = case["n_inst"], case["n_agents"], case["steps"]
    ex = BatchedExpert(case["grids"], n_inst, n, T, seed=case["seed"], swap=case["swap"], lifelong=True)
    ex.reset(torch.from_numpy(case["pos"]), torch.from_numpy(case["goal"]), torch.from_numpy(case["queue"]))
    pos, goal, done = [x.cpu().numpy().copy() for x in ex.env.sync_state()]
    assert np.array_equal(pos, case["pos"]) and np.array_equal(goal, case["goal"]) and not done.any()
    goals, counted = [goal], np.zeros((n_inst, T), np.int64)
    for t in range(T):
        ex.step()
        after, goal_after, done_after = [x.cpu().numpy().copy() for x in ex.env.sync_state()]
        try:
            ck.check_transition(case["grids"], pos, ex.actions.cpu().numpy(), ex.planned().cpu().numpy(), after, done != 0)
        except AssertionError as e:
            raise AssertionError(f"step {t}: {e}") from None
        counted[:, t] = (after == goal).all(-1).sum(1)
        assert np.array_equal(ex.arrivals()[:, t].cpu().numpy(), counted[:, t]), f"arrivals of step {t}"
        pos, goal, done = after, goal_after, done_after
        goals.append(goal)
    assert (done == 2).all()
    log, lens = [x.cpu().numpy() for x in ex.log()]
    assert (lens == T).all() and ((log >= 0) & (log <= 4)).all()
    assert np.array_equal(ex.arrivals().cpu().numpy(), counted)
    reached = ex.env.goals_reached().cpu().numpy()
    assert np.array_equal(reached.sum(1), counted.sum(1))
    hist = np.stack(goals)                                      # [T + 1, inst, agent, 2]
    targets = ex.targets()
    for i in range(n_inst):
        paths = dt.agent_paths(case["pos"][i], log[i])
        assert np.array_equal(paths[:, -1], pos[i])
        assert [len(tg) for tg in targets[i]] == (reached[i] + 1).tolist()
        assert np.array_equal(dt.goal_positions(paths, targets[i]), hist[:, i].transpose(1, 0, 2)), f"instance {i}"
    thr = ex.throughput().cpu().numpy()
    assert np.array_equal(thr, counted.sum(1).astype(np.float32) / np.float32(T))
    assert (thr > 0).all(), "an instance without a single arrival"
