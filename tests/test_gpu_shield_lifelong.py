"""The collision shield on lifelong episodes on the device against its restatement
(tests/shield_lifelong_ref.py): bit equality after every step (actions, planned cells, env positions and goals, overrides, the `first`
copy; `since` shows through the next step's order) and at the end (the arrivals log, throughput, the env's counts and lengths) on the
non-swap shapes of expert_lifelong_ref.gpu_cases() with seeded goal-seeking logits; the shield behind the tiny policy in BatchedRunner
(graph, recorder, retire mode, shards, a second episode, steps beyond the cap, determinism); the switch back to the plain shield; the
new refusals; the evaluation branch.  No tolerance anywhere: everything is integer state or bit patterns."""
import os

import numpy as np
import pytest

from tests import expert_lifelong_ref as lr
from tests import expert_ref as er
from tests import shield_lifelong_ref as slr
from tests import shield_ref as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = slr.cases()


def make_shield(case):
    import torch
    from mapf_gpt_amd.expert import BatchedExpert
    ex = BatchedExpert(case["grids"], case["n_inst"], case["n_agents"], case["steps"], shield=True, shield_lifelong=True)
    ex.reset(torch.from_numpy(case["pos"]), torch.from_numpy(case["goal"]), torch.from_numpy(case["queue"]))
    return ex, slr.new_ref(case)


def device_step(ex, bits, first):
    """One shield_step with the logits given as bit patterns [inst, agent, width] -> (actions, planned, pos, goal, done, overrides,
    first copy) as numpy."""
    import torch
    width = bits.shape[-1]
    logits = torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32).reshape(-1, width))
    act = ex.shield_step(logits, torch.from_numpy(np.asarray(first, np.int32))).cpu().numpy().copy()
    pos, goal, done = ex.env.sync_state()
    return (act, ex.planned().cpu().numpy(), pos.cpu().numpy(), goal.cpu().numpy(), done.cpu().numpy(), ex.shield_overrides().cpu().numpy(),
            ex.shield_first().cpu().numpy())


def assert_steps_equal(ex, ref, steps, seed=slr.SEED):
    rng = np.random.default_rng(seed)
    for t in range(steps):
        bits, first = slr.step_inputs(ref, rng, t)                         # rows of 7 logits on even steps, of 5 on odd ones
        assert not ref.done.any()                                          # truncation only: every instance plans at every step
        want_act, want_planned = ref.step(bits, first)
        act, planned, pos, goal, done, over, first_copy = device_step(ex, bits, first)
        assert np.array_equal(act, want_act), f"actions differ at step {t}"
        assert np.array_equal(planned, want_planned), f"planned cells differ at step {t}"
        assert np.array_equal(pos, ref.pos), f"env positions differ at step {t}"
        assert np.array_equal(pos, planned), f"the env left an agent off its planned cell at step {t}"
        assert np.array_equal(goal, ref.goal), f"env goals differ at step {t}"
        assert np.array_equal(done, ref.done), f"done flags differ at step {t}"
        assert np.array_equal(over, ref.overrides), f"overrides differ at step {t}"
        assert np.array_equal(first_copy, first), f"the first copy differs at step {t}"


def assert_final_state(ex, ref):
    arr = ex.arrivals()
    assert arr.dtype.is_floating_point is False and arr.element_size() == 2 and tuple(arr.shape) == (ref.n_inst, ref.max_steps)
    assert np.array_equal(arr.cpu().numpy(), ref.arrivals_log())
    reached = ex.env.goals_reached().cpu().numpy()
    assert np.array_equal(reached, ref.reached)
    assert np.array_equal(arr.cpu().numpy().sum(1), reached.sum(1))       # the env's own count, the figure behind avg_throughput
    assert np.array_equal(ex.throughput().cpu().numpy(), ref.throughput())
    assert (ex.env.sync_state()[2].cpu().numpy() == 2).all()
    assert np.array_equal(ex.metrics()[:, 4].cpu().numpy(), np.full(ref.n_inst, ref.max_steps, np.float32))


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_step_equals_the_restatement(name):
    case = CASES[name]
    ex, ref = make_shield(case)
    assert_steps_equal(ex, ref, case["steps"])
    assert_final_state(ex, ref)
    assert ref.reached.sum(1).min() >= 1 and (ref.overrides.min() >= 1 or case["n_agents"] < 8)


def test_a_second_episode_then_the_plain_shield_again():
    """reset() with another queue clears held / live / arrivals / steps; set_shield_lifelong(0) between episodes restores the plain
    shield exactly: a one-shot episode on the same context equals shield_ref.RefShield."""
    import torch
    from mapf_gpt_amd import _lib
    case = CASES["shared5"]
    ex, ref = make_shield(case)
    assert_steps_equal(ex, ref, case["steps"])
    other = dict(case, queue=np.ascontiguousarray(case["queue"][:, ::-1, ::-1][:, :, :5]))       # other cells, another queue length
    ex.reset(torch.from_numpy(other["pos"]), torch.from_numpy(other["goal"]), torch.from_numpy(other["queue"]))
    ref = slr.new_ref(other)
    assert_steps_equal(ex, ref, case["steps"], seed=slr.SEED + 1)
    assert_final_state(ex, ref)
    allocs = _lib.mem_debug()[0]
    ex.set_shield_lifelong(False)                                         # between episodes: every instance is done
    assert _lib.mem_debug()[0] == allocs - 4                              # held, live, arrivals, steps
    assert _lib.lib().mgpt_expert_copy_arrivals(ex._h, _lib.ptr(torch.empty(8, device="cuda")), None) == _lib.ERR_STATE
    one = er.random_case(12, 12, 0.2, 5, 8, case["steps"], seed=8)        # the one-shot case shared5 was made from: the context's grid
    assert np.array_equal(one["grids"], case["grids"])
    ex.reset(torch.from_numpy(one["pos"]), torch.from_numpy(one["goal"]))
    assert not ex.env.lifelong
    plain = sr.RefShield(one["grids"], 5, 8, case["steps"])
    plain.reset(one["pos"], one["goal"])
    rng = np.random.default_rng(3)
    for t in range(12):
        bits, first = sr.random_logits(rng, 5, 8), rng.integers(0, 5, size=(5, 8))
        skip = plain.done != 0
        want_act, want_planned = plain.step(bits, first)
        act, planned, pos, _, done, over, _ = device_step(ex, bits, first)
        assert np.array_equal(act, want_act) and np.array_equal(planned[~skip], want_planned[~skip]), t
        assert np.array_equal(pos, plain.pos) and np.array_equal(done, plain.done) and np.array_equal(over, plain.overrides), t


def test_one_context_walked_through_the_modes_equals_a_fresh_context_in_each():
    """The planner's and the shield's lifelong modes share one state (held / live / arrivals / steps).  One context goes planner
    lifelong -> one-shot planner -> shield -> lifelong shield -> shield -> one-shot planner -> planner lifelong, with a reset and a whole
    6-step episode after every switch (every instance is then done by truncation, so the next switch is allowed); after every episode
    its log, lengths, planned cells, env positions and, where the mode has them, arrivals and overrides are those of a context created
    directly in that mode and given the same inputs."""
    import torch
    from mapf_gpt_amd import _lib
    from mapf_gpt_amd.expert import BatchedExpert
    case = lr.random_case(12, 12, 0.2, 2, 3, 6, seed=21, Q=4)
    pos, goal, queue = (torch.from_numpy(case[k]) for k in ("pos", "goal", "queue"))
    mk = lambda **kw: BatchedExpert(case["grids"], 2, 3, 6, seed=case["seed"], inst_offset=case["inst_offset"], **kw)
    modes = {"lifelong": dict(lifelong=True), "plain": {}, "shield": dict(shield=True), "shield_lifelong": dict(shield=True, shield_lifelong=True)}

    def shield_inputs(mode):                                              # the logits of the episode, from the mode's restatement
        if mode == "shield_lifelong":
            ref = slr.new_ref(case)
        else:
            ref = sr.RefShield(case["grids"], 2, 3, 6)
            ref.reset(case["pos"], case["goal"])
        rng, out = np.random.default_rng(slr.SEED), []
        for t in range(6):
            out.append(slr.step_inputs(ref, rng, t))
            ref.step(*out[-1])
        return out

    inputs = {mode: shield_inputs(mode) for mode in ("shield", "shield_lifelong")}

    def episode(ex, mode):
        ex.reset(pos, goal, queue if "lifelong" in mode else None)
        if "shield" in mode:
            for bits, first in inputs[mode]:
                device_step(ex, bits, first)
        else:
            ex.run(6)
        log, lens = ex.log()
        out = {"log": log, "lens": lens, "planned": ex.planned(), "pos": ex.env.sync_state()[0], "done": ex.env.sync_state()[2]}
        if "lifelong" in mode:
            out["arrivals"] = ex.arrivals()
        else:
            with pytest.raises(_lib.MGPTError):                           # no arrivals log in a one-shot mode, whatever came before
                ex.arrivals()
        if "shield" in mode:
            out["overrides"] = ex.shield_overrides()
        return {k: v.cpu().numpy().copy() for k, v in out.items()}

    fresh = {mode: episode(mk(**kw), mode) for mode, kw in modes.items()}
    assert fresh["lifelong"]["arrivals"].sum() > 0 and fresh["shield_lifelong"]["arrivals"].sum() > 0 and fresh["shield_lifelong"]["overrides"].sum() > 0
    ex = mk()
    walk = [("lifelong", lambda: ex.set_lifelong(True)), ("plain", lambda: ex.set_lifelong(False)), ("shield", lambda: ex.set_shield(True)),
            ("shield_lifelong", lambda: ex.set_shield_lifelong(True)), ("shield", lambda: ex.set_shield_lifelong(False)),
            ("plain", lambda: ex.set_shield(False)), ("lifelong", lambda: ex.set_lifelong(True))]
    for leg, (mode, switch) in enumerate(walk):
        switch()
        got = episode(ex, mode)
        assert (got["done"] != 0).all(), (leg, mode)
        assert got.keys() == fresh[mode].keys()
        for k, want in fresh[mode].items():
            assert np.array_equal(got[k], want), f"{k} differs from a fresh {mode} context's on leg {leg} of the walk"


# ---- through the policy ---------------------------------------------------------------------------------------------------------------
N_INST, N_AGENTS, POLICY_STEPS, Q = 2, 8, 16, 4
_cache = {}


def _policy_case():
    if "case" not in _cache:
        import torch
        from mapf_gpt_amd.model import build_model
        case = lr.random_case(12, 12, 0.2, 4, N_AGENTS, POLICY_STEPS, seed=11, Q=Q)              # instances 0..3: the shard test takes 2..3
        _cache["case"] = dict(case, net=build_model("tiny", seed=0, max_rows=4 * N_AGENTS, precision="f32"),
                              t_pos=torch.from_numpy(case["pos"]), t_goal=torch.from_numpy(case["goal"]), t_queue=torch.from_numpy(case["queue"]))
    return _cache["case"]


def _runner(lo=0, hi=N_INST, queue=None, **kw):
    from mapf_gpt_amd.runner import BatchedRunner
    C = _policy_case()
    run = BatchedRunner(C["grids"], hi - lo, N_AGENTS, C["net"], max_episode_steps=POLICY_STEPS, seed=3, do_sample=True, precision="f32",
                        row_offset=lo * N_AGENTS, shield="pibt", shield_lifelong=True, **kw)
    run.reset(C["t_pos"][lo:hi], C["t_goal"][lo:hi], goal_queue=C["t_queue"][lo:hi] if queue is None else queue)
    return run


def _state(run):
    pos, goal, done = run.env.sync_state()
    return (run.actions.cpu().numpy().copy(), pos.cpu().numpy().copy(), goal.cpu().numpy().copy(), done.cpu().numpy().copy(),
            run.shield_overrides().cpu().numpy(), run.arrivals().cpu().numpy(), run.env.goals_reached().cpu().numpy())


def _record(run, steps=POLICY_STEPS):
    """-> per step (actions, positions, goals, done, overrides, arrivals log, the env's counts) as numpy."""
    out = []
    for _ in range(steps):
        run.step()
        out.append(_state(run))
    return out


def _eager():
    if "eager" not in _cache:
        _cache["eager"] = _record(_runner())
    return _cache["eager"]


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for t, (a, b) in enumerate(zip(got, want)):
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), (what, t)


def test_through_the_policy_every_step_equals_the_restatement():
    """The restatement applied to the device's own logits and `first`; the fields the plan reads are those the step's own update_agents
    rebuilt at its head."""
    C = _policy_case()
    run = _runner()
    ref = slr.RefShieldLifelong(C["grids"], N_INST, N_AGENTS, POLICY_STEPS)
    ref.reset(C["pos"][:N_INST], C["goal"][:N_INST], C["queue"][:N_INST])
    for t in range(POLICY_STEPS):
        run.step()
        logits, first, actions, planned = (x.cpu().numpy() for x in run.shield_state())
        want_act, want_planned = ref.step(sr.bits_of(logits).reshape(N_INST, N_AGENTS, 67), first)
        assert np.array_equal(actions, want_act), f"actions differ at step {t}"
        assert np.array_equal(planned, want_planned), f"planned cells differ at step {t}"
        pos, goal, done = (x.cpu().numpy() for x in run.env.sync_state())
        assert np.array_equal(pos, ref.pos) and np.array_equal(goal, ref.goal) and np.array_equal(done, ref.done), t
        assert np.array_equal(pos, planned), "the env left an agent off its planned cell"
        assert np.array_equal(run.shield_overrides().cpu().numpy(), ref.overrides), t
        assert np.array_equal(run.arrivals().cpu().numpy(), ref.arrivals_log()), t
    assert np.array_equal(run.env.goals_reached().cpu().numpy(), ref.reached)
    assert np.array_equal(run.arrivals().cpu().numpy().sum(1), ref.reached.sum(1))
    assert np.array_equal(run.metrics()[:, 4].cpu().numpy(), np.full(N_INST, POLICY_STEPS, np.float32))
    assert ref.overrides.sum() > 0                                        # the synthetic policy does run into conflicts
    want = _eager()                                                       # (and the recorded eager run is this run)
    assert np.array_equal(want[-1][1], ref.pos) and np.array_equal(want[-1][5], ref.arrivals_log())


def test_graph_replay_equals_eager_and_two_runs_give_the_same_bits():
    want = _eager()
    for kw in ({"use_graph": True}, {}):
        _assert_same(_record(_runner(**kw)), want, kw)


def test_steps_replayed_beyond_the_cap_write_nothing():
    """Exactly T steps, then two more replays of the captured step: the arrivals log is unchanged (the kernel's own bound; every instance
    is done, so `live` keeps the step counter at T) and nothing else is disturbed."""
    run = _runner(use_graph=True)
    got = _record(run)
    _assert_same(got, _eager(), "graph")
    planned = run._shield.planned().cpu().numpy()
    for _ in range(2):
        run.step()
    after = _state(run)
    assert all(np.array_equal(x, y) for x, y in zip(after[1:], got[-1][1:]))                    # positions .. the env's counts
    assert np.array_equal(run._shield.planned().cpu().numpy(), planned)
    assert (after[3] == 2).all() and np.array_equal(run.metrics()[:, 4].cpu().numpy(), np.full(N_INST, POLICY_STEPS, np.float32))


def test_the_recorder_changes_no_bit_and_records_the_envs_positions():
    C = _policy_case()
    run = _runner(record=True)
    got = _record(run)
    _assert_same(got, _eager(), "record")
    pos, act, lens = (x.cpu().numpy() for x in run.trajectory())
    assert np.array_equal(pos[0], C["pos"][:N_INST]) and (lens == POLICY_STEPS).all()
    for t in range(POLICY_STEPS):
        assert np.array_equal(pos[t + 1], got[t][1]) and np.array_equal(act[t], got[t][0]), t


def test_retire_mode_equals_the_plain_run():
    """Nothing retires before truncation, so every bit is the plain run's."""
    run = _runner(retire_done=True, poll_every=4)
    _assert_same(_record(run), _eager(), "retire")
    assert run.live_instances == N_INST


def test_a_shard_equals_its_slice_of_the_unsharded_run():
    whole = _record(_runner(0, 4), 8)
    shard = _record(_runner(2, 4), 8)
    for t, (a, b) in enumerate(zip(whole, shard)):
        assert all(np.array_equal(x[2:], y) for x, y in zip(a, b)), t


def test_a_second_reset_with_another_queue():
    C = _policy_case()
    run = _runner()
    run.run(5)
    other = C["t_queue"][:N_INST].flip(1).flip(2)[:, :, :3].contiguous()                       # other cells, another queue length
    run.reset(C["t_pos"][:N_INST], C["t_goal"][:N_INST], goal_queue=other)
    ref = slr.RefShieldLifelong(C["grids"], N_INST, N_AGENTS, POLICY_STEPS)
    ref.reset(C["pos"][:N_INST], C["goal"][:N_INST], other.numpy())
    for t in range(POLICY_STEPS):
        run.step()
        logits, first, actions, _ = (x.cpu().numpy() for x in run.shield_state())
        want_act, _ = ref.step(sr.bits_of(logits).reshape(N_INST, N_AGENTS, 67), first)
        assert np.array_equal(actions, want_act), t
    assert np.array_equal(run.arrivals().cpu().numpy(), ref.arrivals_log()) and np.array_equal(run.env.goals_reached().cpu().numpy(), ref.reached)
    assert np.array_equal(run.shield_overrides().cpu().numpy(), ref.overrides)
    assert np.array_equal(run.env.sync_state()[1].cpu().numpy(), ref.goal)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_the_setter_is_refused_in_the_middle_of_a_replayed_episode():
    """As set_shield: after the expert alone is reset and ONE replayed step has run, the switch is MGPT_ERR_STATE; right after a reset it
    is allowed."""
    from mapf_gpt_amd import _lib
    L = _lib.lib()
    run = _runner(use_graph=True)
    for _ in range(3):                                                    # eager, capture, replay
        run.step()
    run._shield.reset_shield()
    assert L.mgpt_expert_set_shield_lifelong(run._shield._h, 1) == _lib.OK                      # nothing has run since its reset (and it is on)
    run.step()                                                            # a replayed step only
    assert L.mgpt_expert_set_shield_lifelong(run._shield._h, 0) == _lib.ERR_STATE
    assert b"mgpt_expert_set_shield_lifelong in the middle of an episode" in L.mgpt_last_error()


def test_refusals_return_the_stated_status():
    import torch
    from mapf_gpt_amd import _lib
    from mapf_gpt_amd.expert import BatchedExpert
    from mapf_gpt_amd.runner import BatchedRunner
    L = _lib.lib()
    case = CASES["grids3"]
    pos, goal, queue = (torch.from_numpy(case[k]) for k in ("pos", "goal", "queue"))
    mk = lambda **kw: BatchedExpert(case["grids"], 3, 8, 8, **kw)
    # the setter: on a context that is not in shield mode, with a bad value
    for kw in ({}, {"lifelong": True}):
        ex = mk(**kw)
        assert L.mgpt_expert_set_shield_lifelong(ex._h, 1) == _lib.ERR_STATE and b"mgpt_expert_set_shield(ex, 1) must precede" in L.mgpt_last_error()
        assert L.mgpt_expert_set_shield_lifelong(ex._h, 0) == _lib.ERR_STATE
    ex = mk(shield=True)
    assert L.mgpt_expert_set_shield_lifelong(ex._h, 2) == _lib.ERR_ARG
    # the arrivals of a plain shield; what the plain shield refuses stays refused, before and after the switch
    ex.reset(pos, goal)
    out = torch.empty((3, 8), dtype=torch.int16, device="cuda")
    assert L.mgpt_expert_copy_arrivals(ex._h, _lib.ptr(out), _lib.stream_ptr()) == _lib.ERR_STATE
    assert L.mgpt_expert_set_lifelong(ex._h, 1) == _lib.ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="goal_queue"):
        ex.reset(pos, goal, goal_queue=queue)
    assert L.mgpt_expert_set_shield_lifelong(ex._h, 1) == _lib.OK
    ex.shield_lifelong = True
    assert L.mgpt_expert_set_lifelong(ex._h, 1) == _lib.ERR_UNSUPPORTED
    assert L.mgpt_expert_set_search(ex._h, 16, 0, 0) == _lib.ERR_UNSUPPORTED and L.mgpt_expert_set_swap(ex._h, 1) == _lib.ERR_UNSUPPORTED
    # reset / shield / commit on an env without queues, or before the reset that must follow the switch
    logits = torch.zeros((24, 5), device="cuda")
    args = lambda e: (e._h, _lib.ptr(logits), 5, None, None, _lib.ptr(e.actions.view(-1)), _lib.stream_ptr())
    assert L.mgpt_expert_shield(*args(ex)) == _lib.ERR_STATE              # a reset must follow the switch
    assert L.mgpt_expert_shield_commit(ex._h, _lib.stream_ptr()) == _lib.ERR_STATE
    assert L.mgpt_expert_reset(ex._h, _lib.stream_ptr()) == _lib.ERR_STATE
    assert b"lifelong shield is on (mgpt_expert_set_shield_lifelong): mgpt_env_set_lifelong must come first" in L.mgpt_last_error()
    with pytest.raises(ValueError, match="goal_queue"):
        ex.reset(pos, goal)
    ex.reset(pos, goal, goal_queue=queue)
    assert L.mgpt_expert_shield(*args(ex)) == _lib.OK                     # (an episode has begun)
    ex.env.set_lifelong(None)
    assert L.mgpt_expert_shield(*args(ex)) == _lib.ERR_STATE and b"mgpt_env_set_lifelong must come first" in L.mgpt_last_error()
    ex.env.set_lifelong(queue)
    assert L.mgpt_expert_set_shield_lifelong(ex._h, 0) == _lib.ERR_STATE and b"middle of an episode" in L.mgpt_last_error()
    assert L.mgpt_expert_set_shield(ex._h, 0) == _lib.ERR_STATE
    # mgpt_expert_set_shield(ex, 0) releases the four buffers with the shield's own three
    ex = mk(shield=True, shield_lifelong=True)
    allocs = _lib.mem_debug()[0]
    ex.set_shield(False)
    assert _lib.mem_debug()[0] == allocs - 7 and ex.shield_lifelong is False
    ex.set_shield(True)
    ex.reset(pos, goal)
    assert L.mgpt_expert_copy_arrivals(ex._h, _lib.ptr(out), _lib.stream_ptr()) == _lib.ERR_STATE
    # the Python side
    C = _policy_case()
    with pytest.raises(ValueError, match="shield_lifelong"):
        mk(shield_lifelong=True)
    with pytest.raises(ValueError, match="shield_lifelong"):
        BatchedRunner(C["grids"], N_INST, N_AGENTS, C["net"], max_episode_steps=POLICY_STEPS, precision="f32", shield_lifelong=True)
    run = _runner()
    with pytest.raises(ValueError, match="goal_queue"):
        run.reset(C["t_pos"][:N_INST], C["t_goal"][:N_INST])
    plain = BatchedRunner(C["grids"], N_INST, N_AGENTS, C["net"], max_episode_steps=POLICY_STEPS, precision="f32", shield="pibt")
    with pytest.raises(RuntimeError, match="shield_lifelong"):
        plain.arrivals()
    with pytest.raises(NotImplementedError):
        plain.reset(C["t_pos"][:N_INST], C["t_goal"][:N_INST], goal_queue=C["t_queue"][:N_INST])


# ---- evaluation -------------------------------------------------------------------------------------------------------------------------
def _eval_cfg(on_target, algorithms):
    from mapf_gpt_amd import evaluation as ev
    cfg = ev.load_yaml(os.path.join(ROOT, "eval_configs", "00-smoke", "00-smoke.yaml"))
    cfg["environment"]["seed"] = {"grid_search": [0]}
    cfg["environment"]["num_agents"] = {"grid_search": [8]}
    cfg["environment"]["max_episode_steps"] = 16
    cfg["environment"]["on_target"] = on_target
    cfg.pop("results_views", None)
    algo = dict(cfg["algorithms"]["MAPF-GPT-2M"], path_to_weights="synthetic:tiny", precision="f32")
    cfg["algorithms"] = {name: dict(algo, **extra) for name, extra in algorithms.items()}
    return cfg


def test_evaluation_runs_restart_groups_behind_the_lifelong_shield():
    from mapf_gpt_amd import evaluation as ev
    seen = []

    def on_batch(info):
        run = info["runner"]
        assert run.shield_lifelong and info["on_target"] == "restart"
        seen.append((run.env.goals_reached().sum(1).cpu().numpy(), run.arrivals().cpu().numpy().sum(1), run.shield_overrides().cpu().numpy()))

    cfg = _eval_cfg("restart", {"shielded": {"shield": "pibt", "shield_lifelong": True}})
    res = ev.evaluation(cfg, print_fn=lambda *_: None, on_batch=on_batch)
    reached, arrived, over = (np.concatenate(x) for x in zip(*seen))
    assert len(res) == len(reached) == 2 and np.array_equal(reached, arrived)
    for r, n, o in zip(res, reached, over):
        m = r["metrics"]
        assert set(m) == {"avg_throughput", "ep_length", "shield_overrides", "runtime"} and m["ep_length"] == 16
        assert m["avg_throughput"] == float(np.float32(n) / np.float32(16))                   # the runner's own count (16: a power of two, exact)
        assert 0.0 <= m["shield_overrides"] <= 1.0 and m["shield_overrides"] == float(np.float32(o)) / (16.0 * 8)
    assert any(r["metrics"]["shield_overrides"] > 0 for r in res)
    with pytest.raises(NotImplementedError):                              # without the key the restart group raises as before
        ev.evaluation(_eval_cfg("restart", {"shielded": {"shield": "pibt"}}), print_fn=lambda *_: None)


def test_evaluation_on_a_nothing_config_is_the_plain_shield():
    from mapf_gpt_amd import evaluation as ev
    cfg = _eval_cfg("nothing", {"shielded": {"shield": "pibt"}, "both": {"shield": "pibt", "shield_lifelong": True}})
    res = ev.evaluation(cfg, print_fn=lambda *_: None, on_batch=lambda info: None if not info["runner"].shield_lifelong else pytest.fail("lifelong"))
    strip = lambda name: [{k: v for k, v in r["metrics"].items() if k != "runtime"} for r in res if r["algorithm"] == name]
    assert len(strip("both")) == 2 and strip("both") == strip("shielded")
    assert all("shield_overrides" in m and "CSR" in m for m in strip("both"))
