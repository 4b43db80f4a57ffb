"""The expert's lifelong mode on the device against its restatement (tests/expert_lifelong_ref.py): bit equality
after every step (actions, planned cells, env positions and goals, arrivals so far -- the order by `since` shows through the actions)
and at the end (logs, lengths, the arrivals log, targets, throughput) on the shapes of expert_lifelong_ref.gpu_cases(); sharding,
determinism, a second episode, the switch back to one-shot planning, the refusals, the evaluation branch, the dataset tokenizer on the
logged records and the command-line tool."""
import json
import os

import numpy as np
import pytest

from tests import expert_lifelong_ref as lr
from tests import expert_ref as er

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = lr.gpu_cases()
_REFS = {}


def make_expert(case, reset=True):
    import torch
    from mapf_gpt_amd.expert import BatchedExpert
    ex = BatchedExpert(case["grids"], case["n_inst"], case["n_agents"], case["steps"], seed=case["seed"], inst_offset=case["inst_offset"],
                       swap=case["swap"], lifelong=True)
    if reset:
        ex.reset(torch.from_numpy(case["pos"]), torch.from_numpy(case["goal"]), torch.from_numpy(case["queue"]))
    return ex


def final_ref(name):
    """The restatement after the case's whole episode (computed once, read only)."""
    if name not in _REFS:
        _REFS[name] = lr.run_case(CASES[name])
    return _REFS[name]


def assert_final_state(ex, ref):
    log, lens = ex.log()
    want_log, want_len = ref.log()
    assert (want_len == ref.max_steps).all()                    # truncation only
    assert np.array_equal(lens.cpu().numpy(), want_len)
    assert np.array_equal(log.cpu().numpy(), want_log)
    arr = ex.arrivals()
    assert arr.dtype.is_floating_point is False and tuple(arr.shape) == (ref.n_inst, ref.max_steps)
    assert np.array_equal(arr.cpu().numpy(), ref.arrivals_log())
    assert np.array_equal(arr.cpu().numpy().sum(1), ex.env.goals_reached().cpu().numpy().sum(1))
    assert ex.targets() == ref.targets()
    assert np.array_equal(ex.throughput().cpu().numpy(), ref.throughput())
    pos, goal, done = ex.env.sync_state()
    assert np.array_equal(pos.cpu().numpy(), ref.pos) and np.array_equal(goal.cpu().numpy(), ref.goal) and (done.cpu().numpy() == 2).all()
    assert np.array_equal(ex.metrics()[:, 4].cpu().numpy(), want_len.astype(np.float32))


def assert_steps_equal(ex, ref, steps):
    for t in range(steps):
        ex.step()
        act, planned = ref.step()
        pos, goal, done = ex.env.sync_state()
        assert np.array_equal(ex.actions.cpu().numpy(), act), f"actions differ at step {t}"
        assert np.array_equal(ex.planned().cpu().numpy(), planned), f"planned cells differ at step {t}"
        assert np.array_equal(pos.cpu().numpy(), ref.pos), f"env positions differ at step {t}"
        assert np.array_equal(goal.cpu().numpy(), ref.goal), f"env goals differ at step {t}"
        assert np.array_equal(ex.env.goals_reached().cpu().numpy(), ref.reached), f"arrival counts differ at step {t}"
        assert np.array_equal(done.cpu().numpy(), ref.done), f"done flags differ at step {t}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_step_equals_the_restatement(name):
    case = CASES[name]
    ex = make_expert(case)
    ref = lr.new_ref(case)
    assert_steps_equal(ex, ref, case["steps"])
    assert_final_state(ex, ref)


def test_a_shard_equals_the_same_instances_of_the_unsharded_run():
    shard = CASES["offset7"]
    whole = lr.random_case(12, 12, 0.2, 10, 8, 40, seed=10)
    for k in ("pos", "goal", "queue"):
        assert np.array_equal(whole[k][7:], shard[k])
    a, b = make_expert(whole), make_expert(shard)
    a.run(40)
    b.run(40)
    (la, na), (lb, nb) = a.log(), b.log()
    assert np.array_equal(la[7:].cpu().numpy(), lb.cpu().numpy()) and np.array_equal(na[7:].cpu().numpy(), nb.cpu().numpy())
    assert np.array_equal(a.arrivals()[7:].cpu().numpy(), b.arrivals().cpu().numpy())
    assert a.targets()[7:] == b.targets()
    assert_final_state(b, final_ref("offset7"))


def test_two_runs_give_the_same_bits():
    outs = []
    for _ in range(2):
        ex = make_expert(CASES["agents70"])
        ex.run(CASES["agents70"]["steps"])
        log, lens = ex.log()
        outs.append((log.cpu().numpy(), lens.cpu().numpy(), ex.arrivals().cpu().numpy(), ex.env.goals_reached().cpu().numpy(),
                     ex.env.sync_state()[0].cpu().numpy().copy(), ex.env.sync_state()[1].cpu().numpy().copy()))
    for x, y in zip(*outs):
        assert np.array_equal(x, y)


def test_a_second_episode_with_another_queue_and_then_one_shot_planning_again():
    import torch
    case = CASES["shared5"]
    ex = make_expert(case)
    ex.run(case["steps"])
    assert_final_state(ex, final_ref("shared5"))
    other = dict(case, queue=np.ascontiguousarray(case["queue"][:, ::-1, ::-1][:, :, :5]))       # other cells, another queue length
    ex.reset(torch.from_numpy(other["pos"]), torch.from_numpy(other["goal"]), torch.from_numpy(other["queue"]))
    ref = lr.new_ref(other)
    assert_steps_equal(ex, ref, case["steps"])
    assert_final_state(ex, ref)
    ex.set_lifelong(False)                                      # between episodes: every instance is done
    one = er.gpu_cases()["shared5"]
    ex.reset(torch.from_numpy(one["pos"]), torch.from_numpy(one["goal"]))
    assert not ex.env.lifelong
    want = er.run_case(one, steps=0)
    for t in range(one["steps"]):
        ex.step()
        act, planned = want.step()
        pos, _, done = ex.env.sync_state()
        assert np.array_equal(ex.actions.cpu().numpy(), act) and np.array_equal(ex.planned().cpu().numpy(), planned), f"step {t}"
        assert np.array_equal(pos.cpu().numpy(), want.pos) and np.array_equal(done.cpu().numpy(), want.done), f"step {t}"
    log, lens = ex.log()
    assert np.array_equal(log.cpu().numpy(), want.log()[0]) and np.array_equal(lens.cpu().numpy(), want.log()[1])
    assert np.array_equal(ex.metrics().cpu().numpy()[:, :5], want.metrics()[:, :5].astype(np.float32))


def test_steps_beyond_the_cap_write_nothing():
    """The planner-mode twin of the lifelong shield's test of the same name: max_steps + 2 steps; after step max_steps every instance is
    done, `live` keeps the post-step kernel's device step counter at max_steps and the two further steps change none of the arrivals
    log, the action log and the lengths (nor the env's positions and counts)."""
    case = lr.random_case(12, 12, 0.2, 2, 3, 6, seed=21, Q=4)
    ex = make_expert(case)
    ref = lr.new_ref(case)
    assert_steps_equal(ex, ref, case["steps"])
    assert_final_state(ex, ref)

    def state():
        log, lens = ex.log()
        return [x.cpu().numpy().copy() for x in (ex.arrivals(), log, lens, ex.env.sync_state()[0], ex.env.goals_reached())]

    at_cap = state()
    assert (at_cap[2] == case["steps"]).all() and at_cap[0].sum() > 0
    for extra in range(2):
        ex.step()
        assert all(np.array_equal(x, y) for x, y in zip(state(), at_cap)), f"step max_steps + {extra + 1} changed the state"


def test_refusals_and_their_messages():
    import torch
    from mapf_gpt_amd import _lib
    from mapf_gpt_amd.expert import BatchedExpert
    case = CASES["pocket"]
    pos, goal, queue = (torch.from_numpy(case[k]) for k in ("pos", "goal", "queue"))
    ex = BatchedExpert(case["grids"], 1, 2, case["steps"], search="lacam", max_iters=64)
    with pytest.raises(_lib.MGPTError, match="mgpt_expert_set_search") as e:       # lifelong with the search on
        ex.set_lifelong(True)
    assert e.value.code == _lib.ERR_UNSUPPORTED and not ex.lifelong
    ex = make_expert(case, reset=False)
    rc = _lib.lib().mgpt_expert_set_search(ex._h, 64, 0, 0)                        # the search with lifelong on
    assert rc == _lib.ERR_UNSUPPORTED and b"mgpt_expert_set_lifelong" in _lib.lib().mgpt_last_error()
    with pytest.raises(_lib.MGPTError) as e:                                       # refinement needs the search: refused with it
        ex.set_refine(2)
    assert e.value.code == _lib.ERR_STATE
    assert _lib.lib().mgpt_expert_set_lifelong(ex._h, 2) == _lib.ERR_ARG
    with pytest.raises(_lib.MGPTError, match="mgpt_expert_reset") as e:            # the arrivals before a reset
        ex.arrivals()
    assert e.value.code == _lib.ERR_STATE
    ex.env.reset(pos, goal)                                                        # a reset without an env queue
    ex.tok.create_agents(ex.env.pos, ex.env.goal)
    rc = _lib.lib().mgpt_expert_reset(ex._h, _lib.stream_ptr())
    assert rc == _lib.ERR_STATE and b"mgpt_env_set_lifelong must come first" in _lib.lib().mgpt_last_error()
    with pytest.raises(ValueError, match="goal_queue"):
        ex.reset(pos, goal)
    ex.reset(pos, goal, queue)
    ex.run(3)
    for switch in (lambda: ex.set_lifelong(False), lambda: ex.set_swap(True)):     # the middle of an episode
        with pytest.raises(_lib.MGPTError, match="middle of an episode") as e:
            switch()
        assert e.value.code == _lib.ERR_STATE
    assert ex.lifelong
    ex.env.set_lifelong(None)                                                      # the env loses its queues under a running episode
    with pytest.raises(_lib.MGPTError, match="mgpt_env_set_lifelong must come first") as e:
        ex.step()
    assert e.value.code == _lib.ERR_STATE
    plain = BatchedExpert(case["grids"], 1, 2, case["steps"])                      # with the option off the refusal is the old one
    plain.env.set_lifelong(queue)
    plain.env.reset(pos, goal)
    plain.tok.create_agents(plain.env.pos, plain.env.goal)
    rc = _lib.lib().mgpt_expert_reset(plain._h, _lib.stream_ptr())
    assert rc == _lib.ERR_UNSUPPORTED
    assert _lib.lib().mgpt_last_error() == b"the PIBT expert does not plan lifelong (on_target = restart) episodes"
    with pytest.raises(_lib.MGPTError) as e:
        plain.arrivals()
    assert e.value.code == _lib.ERR_STATE


def restart_config(n_agents=8):
    from mapf_gpt_amd import evaluation as ev
    cfg = ev.load_yaml(os.path.join(ROOT, "eval_configs", "00-smoke", "00-smoke.yaml"))
    cfg["environment"]["on_target"] = "restart"
    cfg["environment"]["num_agents"] = n_agents
    cfg["algorithms"] = {"PIBT": {"name": "PIBT", "seed": 2, "lifelong": True}}
    return cfg


def test_evaluation_runs_a_lifelong_pibt_entry_and_its_throughput_is_the_restatements(tmp_path):
    from mapf_gpt_amd import evaluation as ev
    seen = []
    res = ev.evaluation(restart_config(), eval_dir=str(tmp_path), print_fn=lambda *_: None,
                        trace=lambda kind, payload: seen.append(payload) if kind == "reset" else None)
    assert len(res) == 8 and os.path.exists(tmp_path / "PIBT.json") and len(seen) == 1
    b = seen[0]
    assert b["on_target"] == "restart" and b["goal_queue"].shape == (8, 8, ev.LIFELONG_QUEUE, 2)
    ref = lr.RefLifelongExpert(b["grids"], 8, 8, b["max_steps"], seed=2)
    ref.reset(b["pos"], b["goal"], b["goal_queue"])
    ref.run(b["max_steps"])
    for k, r in enumerate(res):
        assert set(r["metrics"]) == {"avg_throughput", "ep_length", "runtime"} and r["algorithm"] == "PIBT"
        assert r["metrics"]["avg_throughput"] == float(ref.throughput()[k]) and r["metrics"]["ep_length"] == b["max_steps"]
    assert sum(r["metrics"]["avg_throughput"] for r in res) > 0


def test_logged_lifelong_records_pass_the_dataset_tokenizer_with_no_episode_dropped():
    from mapf_gpt_amd import dataset_tokenizer as dt, evaluation as ev, maps
    res = ev.evaluation(restart_config(), print_fn=lambda *_: None, log_actions=True)
    assert len(res) == 8
    want_labels = []
    for r in res:
        m = r["metrics"]
        assert "CSR" not in m and len(m["global_lifelong_targets_xy"]) == 8
        T = int(m["ep_length"])
        assert len(m["made_actions"]) == 8 and all(len(a) == T for a in m["made_actions"])
        for g in dt.gt_actions(m["made_actions"]):
            want_labels.extend(g)
    named = {k: "\n".join(v) for k, v in maps.named_maps().items() if k.startswith("validation-")}
    gen = dt.ObservationGenerator(named, res)
    rows, labels = gen.generate_observations_device(0, len(res))
    assert rows.shape == (sum(8 * (int(r["metrics"]["ep_length"]) + 1) for r in res), 256)        # n_agents x (T + 1) rows per episode
    assert labels.cpu().numpy().tolist() == want_labels


def test_cli_writes_a_lifelong_log(tmp_path, capfd):
    import yaml
    from mapf_gpt_amd import expert
    cfg = restart_config()
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    assert expert.main(["--config", str(tmp_path / "cfg.yaml"), "--out", str(tmp_path / "out"), "--lifelong", "--seed", "2"]) == 0
    line = json.loads(capfd.readouterr().out.strip().splitlines()[-1])
    assert set(line) == {"episodes", "rows", "seconds", "lifelong", "arrivals", "throughput"} and line["lifelong"] is True
    with open(tmp_path / "out" / "PIBT.json") as f:
        recs = json.load(f)
    assert line["episodes"] == len(recs) == 8
    assert line["rows"] == sum(8 * (int(r["metrics"]["ep_length"]) + 1) for r in recs)             # every episode counts
    assert line["arrivals"] == sum(len(tg) - 1 for r in recs for tg in r["metrics"]["global_lifelong_targets_xy"]) > 0
    assert line["throughput"] == round(float(np.mean([r["metrics"]["avg_throughput"] for r in recs])), 4)
