"""The device-resident PIBT expert against its restatement (tests/expert_ref.py): bit equality of every step, logs, lengths and
metrics on the shapes of expert_ref.gpu_cases(); determinism, early finishers, unsupported contexts, the evaluation branch, the
dataset tokenizer on the logged records and the command-line tool."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import expert_ref as er

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = er.gpu_cases()
_REFS = {}


def make_expert(case):
    import torch
    from mapf_gpt_amd.expert import BatchedExpert
    ex = BatchedExpert(case["grids"], case["n_inst"], case["n_agents"], case["steps"], seed=case["seed"], inst_offset=case["inst_offset"])
    ex.reset(torch.from_numpy(case["pos"]), torch.from_numpy(case["goal"]))
    return ex


def final_ref(name):
    """The restatement after the case's whole episode (computed once, read only)."""
    if name not in _REFS:
        _REFS[name] = er.run_case(CASES[name])
    return _REFS[name]


def assert_final_state(ex, ref):
    log, lens = ex.log()
    want_log, want_len = ref.log()
    assert np.array_equal(lens.cpu().numpy(), want_len)
    assert np.array_equal(log.cpu().numpy(), want_log)
    got, want = ex.metrics().cpu().numpy(), ref.metrics()
    assert np.array_equal(got[:, :5], want[:, :5].astype(np.float32)), (got, want)
    # avg_agents_density: the device rounds a float64 mean to float32, the restatement sums the same terms in another order in float64:
    # the two float32 values are at most one unit in the last place (2^-23 relative) apart
    assert np.allclose(got[:, 5], want[:, 5].astype(np.float32), rtol=2.0 ** -23, atol=0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_step_equals_the_restatement(name):
    case = CASES[name]
    ex = make_expert(case)
    ref = er.run_case(case, steps=0)
    for t in range(case["steps"]):
        ex.step()
        act, planned = ref.step()
        pos, _, done = ex.env.sync_state()
        assert np.array_equal(ex.actions.cpu().numpy(), act), f"actions differ at step {t}"
        assert np.array_equal(ex.planned().cpu().numpy(), planned), f"planned cells differ at step {t}"
        assert np.array_equal(pos.cpu().numpy(), ref.pos), f"env positions differ at step {t}"
        assert np.array_equal(done.cpu().numpy(), ref.done), f"done flags differ at step {t}"
    assert_final_state(ex, ref)


def test_a_shard_equals_the_same_instances_of_the_unsharded_run():
    shard = CASES["offset7"]
    whole = er.random_case(12, 12, 0.2, 10, 8, 40, seed=10)
    assert np.array_equal(whole["pos"][7:], shard["pos"]) and np.array_equal(whole["goal"][7:], shard["goal"])
    a, b = make_expert(whole), make_expert(shard)
    a.run(40)
    b.run(40)
    (la, na), (lb, nb) = a.log(), b.log()
    assert np.array_equal(la[7:].cpu().numpy(), lb.cpu().numpy()) and np.array_equal(na[7:].cpu().numpy(), nb.cpu().numpy())
    assert np.array_equal(a.metrics()[7:].cpu().numpy(), b.metrics().cpu().numpy())
    assert_final_state(b, final_ref("offset7"))


def test_two_runs_give_the_same_bits():
    outs = []
    for _ in range(2):
        ex = make_expert(CASES["agents70"])
        ex.run(CASES["agents70"]["steps"])
        log, lens = ex.log()
        outs.append((log.cpu().numpy(), lens.cpu().numpy(), ex.metrics().cpu().numpy(), ex.env.sync_state()[0].cpu().numpy().copy()))
    for x, y in zip(*outs):
        assert np.array_equal(x, y)


def test_an_instance_that_finishes_early_stops_logging():
    case = CASES["shared5"]
    ref = final_ref("shared5")
    want_len = ref.log()[1]
    early = [i for i in range(case["n_inst"]) if want_len[i] < 20]
    assert len(early) >= 2 and (want_len == 40).any()           # finishers and one instance that runs to the cap
    ex = make_expert(case)
    ex.run(20)
    log20, len20 = [t.cpu().numpy().copy() for t in ex.log()]
    assert np.array_equal(len20[early], want_len[early])
    ex.run(20)
    log40, len40 = [t.cpu().numpy() for t in ex.log()]
    assert np.array_equal(log40[early], log20[early]) and np.array_equal(len40[early], len20[early])
    assert (log40[early][:, :, 19:] == 0).all()                 # nothing beyond an early finisher's length
    assert np.array_equal(len40, ex.metrics()[:, 4].cpu().numpy().astype(np.int32))      # length = ep_length
    assert (ex.actions[early].cpu().numpy() == 0).all()         # a finished instance's actions are 0
    assert_final_state(ex, ref)


def test_unsupported_contexts_return_the_stated_status():
    import torch
    from mapf_gpt_amd import _lib
    from mapf_gpt_amd.env import RULE_NO_FOLLOW, BatchedEnv
    from mapf_gpt_amd.expert import BatchedExpert
    from mapf_gpt_amd.observation_generator import BatchedTokenizer
    case = CASES["pocket"]
    env = BatchedEnv(case["grids"], 1, 2, 8)
    tok = BatchedTokenizer(case["grids"], 1, 2)
    h = ctypes.c_void_p()
    create = lambda: _lib.lib().mgpt_expert_create(ctypes.byref(h), tok._h, env._h, 0, 0, 8)
    env.set_rules(RULE_NO_FOLLOW)
    assert create() == _lib.ERR_UNSUPPORTED and b"rule" in _lib.lib().mgpt_last_error()
    env.set_rules(0)
    env.set_lifelong(torch.from_numpy(np.broadcast_to(case["goal"][:, :, None, :], (1, 2, 4, 2)).copy()))
    assert create() == _lib.ERR_UNSUPPORTED and b"lifelong" in _lib.lib().mgpt_last_error()
    env.set_lifelong(None)
    assert create() == _lib.OK
    assert _lib.lib().mgpt_expert_step(h, None, None) == _lib.ERR_ARG
    assert _lib.lib().mgpt_expert_destroy(h) == _lib.OK
    other = BatchedTokenizer(case["grids"], 1, 3)               # a tokenizer of another shape
    assert _lib.lib().mgpt_expert_create(ctypes.byref(h), other._h, env._h, 0, 0, 8) == _lib.ERR_ARG
    ex = BatchedExpert(case["grids"], 1, 2, 8)
    with pytest.raises(_lib.MGPTError) as e:                    # step before reset
        ex.step()
    assert e.value.code == _lib.ERR_STATE
    ex.reset(torch.from_numpy(case["pos"]), torch.from_numpy(case["goal"]))
    ex.env.set_rules(RULE_NO_FOLLOW)                            # a rule mask set after create is refused at the step
    with pytest.raises(_lib.MGPTError) as e:
        ex.step()
    assert e.value.code == _lib.ERR_UNSUPPORTED


def smoke_config():
    from mapf_gpt_amd import evaluation as ev
    cfg = ev.load_yaml(os.path.join(ROOT, "eval_configs", "00-smoke", "00-smoke.yaml"))
    cfg["algorithms"]["MAPF-GPT-2M"]["path_to_weights"] = "synthetic:tiny"
    cfg["algorithms"]["PIBT"] = {"name": "PIBT", "seed": 0}
    return cfg


def test_evaluation_runs_a_pibt_algorithm(tmp_path):
    from mapf_gpt_amd import evaluation as ev
    res = ev.evaluation(smoke_config(), eval_dir=str(tmp_path), print_fn=lambda *_: None)
    assert len(res) == 32 and os.path.exists(tmp_path / "PIBT.json") and os.path.exists(tmp_path / "MAPF-GPT-2M.json")
    pibt = [r for r in res if r["algorithm"] == "PIBT"]
    assert len(pibt) == 16
    for r in pibt:
        assert set(r) == {"metrics", "env_grid_search", "algorithm"}
        assert set(r["metrics"]) == {"CSR", "ISR", "SoC", "makespan", "ep_length", "avg_agents_density", "runtime"}
        assert 0 < r["metrics"]["ep_length"] <= 64 and r["metrics"]["CSR"] in (0.0, 1.0)


def test_logged_records_pass_the_dataset_tokenizer():
    from mapf_gpt_amd import dataset_tokenizer as dt, evaluation as ev, maps
    cfg = smoke_config()
    del cfg["algorithms"]["MAPF-GPT-2M"]
    cfg["environment"]["num_agents"] = 8
    res = ev.evaluation(cfg, print_fn=lambda *_: None, log_actions=True)
    assert len(res) == 8
    for r in res:
        m = r["metrics"]
        assert len(m["made_actions"]) == 8 and all(len(a) == int(m["ep_length"]) for a in m["made_actions"])
        assert np.asarray(m["init_positions"]).shape == (8, 2)
    named = {k: "\n".join(v) for k, v in maps.named_maps().items() if k.startswith("validation-")}
    gen = dt.ObservationGenerator(named, res)
    inputs, labels = gen.generate_observations(0, len(res))
    solved = [r for r in res if r["metrics"]["CSR"] >= 1]
    assert solved, "no solved episode to tokenize"
    assert len(inputs) == len(labels) == sum(8 * (int(r["metrics"]["ep_length"]) + 1) for r in solved)
    with pytest.raises(ValueError):
        ev.evaluation(cfg, print_fn=lambda *_: None, log_actions=True, rank=0, world=2)


def test_cli_log_round_trips_through_split_by_map(tmp_path, capfd):
    import yaml
    from mapf_gpt_amd import dataset_build, expert
    cfg = smoke_config()
    cfg["environment"]["num_agents"] = 8
    cfg["environment"]["seed"] = {"grid_search": [0, 1]}
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    with open(tmp_path / "maps.yaml", "w") as f:
        yaml.safe_dump({"tiny-room": "....\n.##.\n....\n"}, f)
    assert expert.main(["--config", str(tmp_path / "cfg.yaml"), "--maps", str(tmp_path / "maps.yaml"), "--out", str(tmp_path / "out")]) == 0
    line = json.loads(capfd.readouterr().out.strip().splitlines()[-1])
    assert set(line) == {"episodes", "solved", "rows", "seconds"} and line["episodes"] == 4
    per_map = dataset_build.split_by_map(str(tmp_path / "out" / "PIBT.json"), str(tmp_path / "temp"))
    assert set(per_map) == {"validation-random-seed-000", "validation-mazes-seed-000"}
    assert all(len(v) == 2 and "made_actions" in v[0]["metrics"] for v in per_map.values())
    assert os.path.exists(tmp_path / "temp" / "validation-mazes-seed-000.json")
    assert line["solved"] == sum(r["metrics"]["CSR"] >= 1 for v in per_map.values() for r in v)
