"""The expert's kernels above 192 agents and at the full depth of the PIBT stack, against their restatements on the cases of
expert_shapes.many_cases() (tests/test_expert_many_cpu.py pins the same cases on the host):

  193, 256, 257 agents in the four modes and 1024 agents (the env's limit: 16 passes of every strided loop) at the two ends of the LDS
  carve, plain PIBT (18 bytes per agent) and the search with the swap rule (32);
  lane_full and lane_shift at 65, 193 and 300 agents in the four modes and at 1024 in the plan kernel: one push through all n agents,
  which fails back (every agent takes its cell back) or succeeds (every agent moves), so the frame array, swp[] and both unwinds run
  through n frames -- the host file asserts that the restatement's recursion reaches depth n, and every step here equals it;
  refinement of a solved 257-agent instance without and with the swap rule; the lifelong planner and the lifelong shield at 257 agents;
  the shield at 193, 257 and 1024 agents with seeded logits, on both lanes at 300 and 1024 with logits that prefer the forward move
  (the PREF = true generator through the same depth), and behind the tiny policy with 257 agents, eager and replayed from a graph.

Every comparison is on integers and bit-exact, through the helpers of the files that own each mode.  After an episode the same context
is reset and runs it again: a reservation or an occupancy entry that a deep unwind left in the workspace would change that second run.
The distance fields of a case are computed once and shared by its restatements (expert_shapes.fields)."""
import numpy as np
import pytest

from tests import expert_checks as ck
from tests import expert_shapes as es
from tests import shield_ref as sh
from tests.test_gpu_expert import assert_final_state
from tests.test_gpu_expert_search import assert_search_equals
from tests.test_gpu_expert_swap import assert_every_step_equals, make_expert

pytestmark = pytest.mark.gpu
CASES = es.many_cases()
LANES = [f"{form}{n}" for form in ("lane_full", "lane_shift") for n in es.LANE_SIZES]
BIG_LANES = [f"{form}{es.LANE_BIG}" for form in ("lane_full", "lane_shift")]
RUNS = ([(name, mode) for name in es.AGENT_CASES for mode in sorted(es.MODES) if name != "agents1024" or mode in ("pibt", "search_swap")]
        + [(name, mode) for name in LANES for mode in sorted(es.MODES)] + [(name, "pibt") for name in BIG_LANES])


def tensors(case, *keys):
    import torch
    return [torch.from_numpy(case[k]) for k in keys]


@pytest.mark.parametrize("name,mode", RUNS)
def test_every_step_equals_the_restatement(name, mode):
    case, m = CASES[name], es.MODES[mode]
    ex = make_expert(case, search=m["search"], swap=m["swap"])
    ref = es.start(name, mode)
    if m["search"]:
        assert_search_equals(ex, ref)
    with es.recursion(case):
        assert_every_step_equals(ex, ref, case["steps"])
    ex.reset(*tensors(case, "pos", "goal"))                     # the same context again: the workspace was left clean
    if m["search"]:
        assert_search_equals(ex, ref)
    ex.run(case["steps"])
    assert_final_state(ex, ref)


@pytest.mark.parametrize("kind", ["refine", "refine_swap"])
def test_refinement_at_257_agents_equals_the_restatement(kind):
    from tests import expert_refine_ref as rr
    from tests.test_gpu_expert_refine import assert_every_step_equals as assert_refined_steps, assert_refine_equals, make_expert as make_refine
    case = CASES["refine257"]
    ex = make_refine(case, kind == "refine_swap", refine_horizon=case["horizon"])
    ref = es.start("refine257", kind)
    assert len(ref.refine_stats()) == len(rr.REFINE_KEYS) and ref.refine_stats()[5][0] >= 1
    assert_refine_equals(ex, ref)
    assert_refined_steps(ex, ref, case)
    ex.reset(*tensors(case, "pos", "goal"))                     # searches and refines again on the same context
    assert_refine_equals(ex, ref)
    ex.run(case["steps"])
    assert_final_state(ex, ref)


def test_the_lifelong_planner_at_257_agents_equals_the_restatement():
    from tests.test_gpu_expert_lifelong import assert_final_state as assert_lifelong_final, assert_steps_equal, make_expert as make_lifelong
    case = CASES["lifelong257"]
    ex = make_lifelong(case)
    ref = es.start("lifelong257", "lifelong")
    assert_steps_equal(ex, ref, case["steps"])
    assert_lifelong_final(ex, ref)                              # the arrivals log: the shuffle sum of every step equals the restatement's count
    assert ref.arrivals_log().sum() >= 1 and len(set(ref.arrivals[0])) > 1
    ex.reset(*tensors(case, "pos", "goal", "queue"))
    ex.run(case["steps"])
    assert_lifelong_final(ex, ref)


def make_shield(name, lifelong=False):
    from mapf_gpt_amd.expert import BatchedExpert
    case = CASES[name]
    ex = BatchedExpert(case["grids"], case["n_inst"], case["n_agents"], case["steps"], shield=True, shield_lifelong=lifelong)
    ex.reset(*tensors(case, *(("pos", "goal", "queue") if lifelong else ("pos", "goal"))))
    return ex, es.start(name, "shield_lifelong" if lifelong else "shield")


@pytest.mark.parametrize("name", ["agents193", "agents257", "agents1024"])
def test_the_shield_with_seeded_logits_equals_the_restatement(name):
    from tests.test_gpu_shield import assert_step, device_step
    case = CASES[name]
    n_inst, n = case["n_inst"], case["n_agents"]
    ex, ref = make_shield(name)
    rng = np.random.default_rng(case["seed"])
    for t in range(case["steps"]):
        width = 5 if t % 2 else 7                               # ld > 5: only the first five values of a row are read
        bits = sh.random_logits(rng, n_inst, n, width)
        first = rng.integers(0, 5, size=(n_inst, n))
        before, skip = ref.pos.copy(), ref.done != 0
        want = ref.step(bits, first)
        got = device_step(ex, bits, first, width)
        assert_step(got, *want, ref, skip, t)
        assert np.array_equal(ex.shield_first().cpu().numpy()[~skip], first[~skip])
        ck.check_transition(case["grids"], before, np.where(skip[:, None], 0, got[0]), np.where(skip[:, None, None], before, got[1]), got[2], skip)
    assert (ref.overrides > 0).all()


@pytest.mark.parametrize("name", [f"{form}{n}" for form in ("lane_full", "lane_shift") for n in (300, es.LANE_BIG)])
def test_the_shield_on_a_lane_equals_the_restatement(name):
    from tests.test_gpu_shield import assert_step, device_step
    case = CASES[name]
    bits, first = es.lane_logits(case)
    for episode in range(2):                                    # the second on the same context: the workspace was left clean
        if episode == 0:
            ex, ref = make_shield(name)
        else:
            ex.reset(*tensors(case, "pos", "goal"))
            ref = es.start(name, "shield")
        for t in range(2):                                      # lane_shift is done after its first step: the second leaves it untouched
            skip = ref.done != 0
            with es.recursion(case):
                want = ref.step(bits, first)
            assert_step(device_step(ex, bits, first), *want, ref, skip, (episode, t))
    assert ref.overrides[0] == (2 * (case["n_agents"] - 1) if name.startswith("lane_full") else 0)


def test_the_lifelong_shield_at_257_agents_equals_the_restatement():
    from tests.test_gpu_shield_lifelong import assert_final_state as assert_shield_final, assert_steps_equal
    case = CASES["lifelong257"]
    ex, ref = make_shield("lifelong257", lifelong=True)
    assert_steps_equal(ex, ref, case["steps"])
    assert_shield_final(ex, ref)
    assert ref.reached.sum() >= 1 and ref.overrides[0] >= 1


def test_through_the_policy_at_257_agents_eager_and_graph_replay_equal_the_restatement():
    """BatchedRunner(shield="pibt") with the tiny model on agents257: the restatement is teacher-forced with the device's logits and
    sampled actions, as tests/test_gpu_shield.py does with 8 agents; the run replayed from a captured graph gives the eager run's bits."""
    from mapf_gpt_amd.model import build_model
    from mapf_gpt_amd.runner import BatchedRunner
    case, steps = CASES["agents257"], 6
    n = case["n_agents"]
    net = build_model("tiny", seed=0, max_rows=n, precision="f32")

    def runner(**kw):
        run = BatchedRunner(case["grids"], 1, n, net, max_episode_steps=steps, seed=3, do_sample=True, precision="f32", shield="pibt", **kw)
        run.reset(*tensors(case, "pos", "goal"))
        return run

    run, ref, eager = runner(), es.start("agents257", "shield"), []
    ref.max_steps = steps
    for t in range(steps):
        before = ref.pos.copy()
        run.step()
        logits, first, actions, planned = (x.cpu().numpy() for x in run.shield_state())
        want_act, want_planned = ref.step(sh.bits_of(logits).reshape(1, n, 67), first)
        assert np.array_equal(actions, want_act), f"actions differ at step {t}"
        assert np.array_equal(planned, want_planned), f"planned cells differ at step {t}"
        pos, _, done = run.env.sync_state()
        assert np.array_equal(pos.cpu().numpy(), ref.pos) and np.array_equal(done.cpu().numpy(), ref.done)
        ck.check_transition(case["grids"], before, actions, planned, ref.pos, np.zeros(1, bool))
        assert np.array_equal(run.shield_overrides().cpu().numpy(), ref.overrides)
        eager.append((actions.copy(), pos.cpu().numpy().copy(), done.cpu().numpy().copy()))
    assert ref.overrides[0] > 0                                 # the synthetic policy does run into conflicts
    graph = runner(use_graph=True)
    for t in range(steps):
        graph.step()
        pos, _, done = graph.env.sync_state()
        got = (graph.actions.cpu().numpy(), pos.cpu().numpy(), done.cpu().numpy())
        assert all(np.array_equal(x, y) for x, y in zip(got, eager[t])), f"graph replay differs from the eager run at step {t}"
    assert np.array_equal(graph.shield_overrides().cpu().numpy(), ref.overrides)
