"""The episode recorder of the step: trajectory() against the env's positions and the runner's actions copied out
after every step, graph = eager, record on = record off, retire mode, the shield, resets, the slot bound, the refusals, records()
through the dataset tokenizer's agent_paths, and evaluation(record=True).  Tiny policy in f32, 2 instances x 8 agents on a 12 x 12 map at
20 % obstacles, 16 steps."""
import ctypes
import os

import numpy as np
import pytest

from tests import expert_ref as er

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_INST, N_AGENTS, T = 2, 8, 16
_cache = {}


def _case():
    if not _cache:
        import torch
        from mapf_gpt_amd.model import build_model
        c = er.random_case(12, 12, 0.2, N_INST, N_AGENTS, T, seed=3)
        _cache.update(grids=c["grids"], pos=torch.from_numpy(c["pos"]), goal=torch.from_numpy(c["goal"]),
                      net=build_model("tiny", seed=0, max_rows=128, precision="f32"))
    return _cache


def _runner(steps=T, **kw):
    from mapf_gpt_amd.runner import BatchedRunner
    C = _case()
    run = BatchedRunner(C["grids"], N_INST, N_AGENTS, C["net"], max_episode_steps=steps, seed=5, do_sample=True, precision="f32", **kw)
    run.reset(C["pos"], C["goal"])
    return run


def _episode(run, steps=T):
    """Step by step: -> (positions [steps + 1, inst, agent, 2] with the reset positions first, actions [steps, inst, agent], metrics)."""
    pos, act = [run.env.sync_state()[0].cpu().numpy().copy()], []
    for _ in range(steps):
        run.step()
        act.append(run.actions.cpu().numpy().copy())
        pos.append(run.env.sync_state()[0].cpu().numpy().copy())
    return np.stack(pos), np.stack(act), run.metrics().cpu().numpy()


def _traj(run):
    return tuple(x.cpu().numpy() for x in run.trajectory())


def _plain():
    """The episode of the runner without the argument, once."""
    if "plain" not in _cache:
        _cache["plain"] = _episode(_runner())
    return _cache["plain"]


def test_trajectory_is_the_env_positions_and_the_runner_actions_of_every_step():
    run = _runner(record=True)
    pos, act, m = _episode(run)
    tp, ta, tl = _traj(run)
    assert tp.dtype == np.int16 and tp.shape == (T + 1, N_INST, N_AGENTS, 2) and ta.dtype == np.int8 and ta.shape == (T, N_INST, N_AGENTS)
    assert np.array_equal(tp[0], _case()["pos"].numpy()), "slot 0 is not the reset positions"
    assert np.array_equal(tp, pos) and np.array_equal(ta, act)
    assert tl.dtype == np.int32 and np.array_equal(tl, m[:, 4].astype(np.int32))
    assert (pos[1:] != pos[:-1]).any() and len(np.unique(act)) > 1


@pytest.mark.parametrize("use_graph", [False, True])
def test_recording_does_not_change_the_episode_and_graph_replay_records_the_same_bits(use_graph):
    want_pos, want_act, want_m = _plain()
    run = _runner(record=True, use_graph=use_graph)
    pos, act, m = _episode(run)
    assert np.array_equal(pos, want_pos) and np.array_equal(act, want_act) and np.array_equal(m, want_m)
    tp, ta, _ = _traj(run)
    assert np.array_equal(tp, want_pos) and np.array_equal(ta, want_act)


def test_record_false_is_the_runner_without_the_argument():
    from mapf_gpt_amd import _lib
    run = _runner(record=False)
    pos, act, m = _episode(run)
    assert all(np.array_equal(a, b) for a, b in zip((pos, act, m), _plain()))
    with pytest.raises(_lib.MGPTError) as e:
        run.trajectory()
    assert e.value.code == _lib.ERR_STATE


def test_a_second_reset_starts_again_at_slot_0_with_zeroed_buffers():
    run = _runner(record=True)
    run.run(T)
    C = _case()
    run.reset(C["pos"].flip(0), C["goal"].flip(0))
    tp, ta, _ = _traj(run)
    assert np.array_equal(tp[0], C["pos"].flip(0).numpy()) and not tp[1:].any() and not ta.any()
    run.run(3)
    tp, ta, _ = _traj(run)
    assert np.array_equal(tp[3], run.env.sync_state()[0].cpu().numpy()) and tp[1:4].any() and not tp[4:].any() and not ta[3:].any()


def test_a_run_of_exactly_t_steps_fills_the_last_slot_and_later_steps_write_nothing():
    """An env of T = 6 steps: the sixth step writes slot 6 of the positions and slot 5 of the actions, the buffers' last; the env is
    truncated then, and a further step finds t >= T on the device and leaves the buffers as they are."""
    run = _runner(steps=6, record=True)
    pos, act, m = _episode(run, 6)
    tp, ta, tl = _traj(run)
    assert tp.shape[0] == 7 and ta.shape[0] == 6 and tl.tolist() == [6] * N_INST
    assert np.array_equal(tp[6], pos[6]) and np.array_equal(ta[5], act[5]) and np.array_equal(tp, pos) and np.array_equal(ta, act)
    run.step()
    run.step()
    tp2, ta2, _ = _traj(run)
    assert np.array_equal(tp2, tp) and np.array_equal(ta2, ta)


def test_step_reset_with_a_counter_above_zero_still_indexes_from_slot_0():
    from mapf_gpt_amd import _lib
    run = _runner(record=True)
    with _lib.on_device(run.device):
        _lib.check(_lib.lib().mgpt_step_reset(run._step, 5, _lib.stream_ptr()))
    pos, act, _ = _episode(run, 4)
    tp, ta, _ = _traj(run)
    assert np.array_equal(tp[:5], pos) and np.array_equal(ta[:4], act) and not tp[5:].any() and not ta[4:].any()
    # the draws are those of steps 5 .. 8, not of 0 .. 3: the counter itself was honoured
    assert not np.array_equal(act, _plain()[1][:4])


def test_retire_mode_records_the_plain_run_up_to_every_length():
    """64 instances x 2 agents with goals next to the starts (tests/test_gpu_retire.py's case b): instances finish all along the run."""
    from mapf_gpt_amd.model import build_model
    from mapf_gpt_amd.runner import BatchedRunner
    from tests.test_gpu_retire import _case as retire_case
    grid, pos, goal = retire_case("b")
    n_inst, n = pos.shape[:2]
    net = build_model("tiny", seed=0, max_rows=n_inst * n, precision="f32")
    mk = lambda **kw: BatchedRunner(grid, n_inst, n, net, max_episode_steps=32, seed=0, do_sample=True, precision="f32", record=True, **kw)
    plain, ret = mk(), mk(retire_done=True, poll_every=4)
    out = []
    for run in (plain, ret):
        run.reset(pos, goal)
        run.run(32)
        out.append(_traj(run) + (run.metrics().cpu().numpy(),))
    (pp, pa, pl, pm), (rp, ra, rl, rm) = out
    assert np.array_equal(pm, rm) and np.array_equal(pl, rl) and np.array_equal(rl, rm[:, 4].astype(np.int32))
    assert 0 < (pl < 32).sum()                                            # instances did finish before the cap
    for i in range(n_inst):
        L = int(pl[i])
        assert np.array_equal(pp[:L + 1, i], rp[:L + 1, i]) and np.array_equal(pa[:L, i], ra[:L, i]), i
        assert (pp[L:, i] == pp[L, i]).all(), "a finished instance moved"


def test_behind_the_shield_the_recorded_actions_are_the_planned_ones():
    from mapf_gpt_amd.runner import moves_from_positions
    run = _runner(record=True, shield="pibt")
    pos, act, m = _episode(run)
    tp, ta, tl = _traj(run)
    assert np.array_equal(tp, pos) and np.array_equal(ta, act)
    assert int(run.shield_overrides().sum()) > 0                          # the planned actions are not the sampled ones throughout
    moves = moves_from_positions(run.trajectory()[0]).cpu().numpy()
    for i in range(N_INST):
        L = int(tl[i])
        assert np.array_equal(moves[:L, i], ta[:L, i]), "the env made a shielded agent wait"
    rec = run.records([{"map_name": "m", "seed": i} for i in range(N_INST)])
    assert all(r["metrics"]["moves"] == r["metrics"]["made_actions"] for r in rec)


def test_records_go_through_agent_paths():
    from mapf_gpt_amd import dataset_tokenizer as dt
    from tests import ddg_ref as dr
    run = _runner(record=True)
    pos, act, m = _episode(run)
    keys = [{"map_name": "m", "seed": i} for i in range(N_INST)]
    rec = run.records(keys, algorithm="policy")
    forced = 0
    for i, r in enumerate(rec):
        mt = r["metrics"]
        L = int(m[i, 4])
        assert r["algorithm"] == "policy" and r["env_grid_search"] == keys[i]
        assert set(mt) == {"CSR", "ISR", "SoC", "makespan", "ep_length", "avg_agents_density", "made_actions", "moves", "init_positions"}
        assert [mt[k] for k in ("CSR", "ISR", "SoC", "makespan", "ep_length")] == [float(v) for v in m[i, :5]]
        assert mt["init_positions"] == pos[0, i].tolist() and mt["made_actions"] == act[:L, i].T.tolist()
        assert mt["moves"] == dr.moves(pos[:L + 1, i])
        assert np.array_equal(dt.agent_paths(mt["init_positions"], mt["moves"]), pos[:L + 1, i].transpose(1, 0, 2))
        forced += not np.array_equal(dt.agent_paths(mt["init_positions"], mt["made_actions"]), pos[:L + 1, i].transpose(1, 0, 2))
    assert forced > 0                                                       # the untrained policy does walk into walls and each other


def test_refusals():
    import torch
    from mapf_gpt_amd import _lib
    L = _lib.lib()
    run = _runner()
    out = torch.empty(((T + 1) * N_INST * N_AGENTS * 2,), dtype=torch.int16, device="cuda")
    assert L.mgpt_step_copy_record(run._step, _lib.ptr(out), None, _lib.stream_ptr()) == _lib.ERR_STATE and b"recording is off" in L.mgpt_last_error()
    assert L.mgpt_step_set_record(None, 1) == _lib.ERR_ARG
    assert L.mgpt_step_copy_record(None, None, None, None) == _lib.ERR_ARG
    n0 = _lib.mem_debug()[0]
    assert L.mgpt_step_set_record(run._step, 1) == _lib.OK and L.mgpt_step_set_record(run._step, 1) == _lib.OK
    assert _lib.mem_debug()[0] == n0 + 3
    assert L.mgpt_step_copy_record(run._step, None, None, _lib.stream_ptr()) == _lib.OK        # either pointer may be NULL
    assert L.mgpt_step_copy_record(run._step, _lib.ptr(out), None, _lib.stream_ptr()) == _lib.OK
    assert L.mgpt_step_set_record(run._step, 0) == _lib.OK and _lib.mem_debug()[0] == n0
    assert L.mgpt_step_copy_record(run._step, _lib.ptr(out), None, _lib.stream_ptr()) == _lib.ERR_STATE
    # switched off again the step is the plain one
    run.reset(_case()["pos"], _case()["goal"])
    assert all(np.array_equal(a, b) for a, b in zip(_episode(run), _plain()))


def test_evaluation_adds_the_three_keys_only_when_asked():
    from mapf_gpt_amd import dataset_tokenizer as dt
    from mapf_gpt_amd import evaluation as ev
    cfg = ev.load_yaml(os.path.join(ROOT, "eval_configs", "00-smoke", "00-smoke.yaml"))
    cfg["environment"]["seed"] = {"grid_search": [0, 1]}
    cfg["environment"]["num_agents"] = {"grid_search": [8]}
    cfg["environment"]["max_episode_steps"] = 16
    cfg.pop("results_views", None)
    cfg["algorithms"] = {"A": dict(cfg["algorithms"]["MAPF-GPT-2M"], path_to_weights="synthetic:tiny", precision="f32")}
    strip = lambda res: [({k: v for k, v in r["metrics"].items() if k != "runtime"}, r["env_grid_search"], r["algorithm"]) for r in res]
    today = strip(ev.evaluation(cfg, print_fn=lambda *_: None))
    off = strip(ev.evaluation(cfg, print_fn=lambda *_: None, record=False))
    assert off == today
    seen = []
    on = strip(ev.evaluation(cfg, print_fn=lambda *_: None, record=True, on_batch=seen.append, log_actions=True))
    assert len(on) == len(today) >= 2
    for (m, key, algo), (m0, key0, algo0) in zip(on, today):
        assert set(m) - set(m0) == {"made_actions", "init_positions", "moves"} and (key, algo) == (key0, algo0)
        assert {k: m[k] for k in m0} == m0
        n = int(m["ep_length"])
        assert len(m["moves"]) == 8 and all(len(a) == n for a in m["moves"] + m["made_actions"])
        assert dt.agent_paths(m["init_positions"], m["moves"]).shape == (8, n + 1, 2)
    assert len(seen) >= 1 and sum(len(b["mine"]) for b in seen) == len(on)
    info = seen[0]
    assert set(info) >= {"runner", "mine", "grids", "pos", "goal", "run_keys", "n_agents", "max_steps", "on_target"}
    assert info["runner"].record and info["n_agents"] == 8 and info["max_steps"] == 16 and info["on_target"] == "nothing"
    with pytest.raises(ValueError):
        ev.evaluation(cfg, print_fn=lambda *_: None, record=True, world=2)
