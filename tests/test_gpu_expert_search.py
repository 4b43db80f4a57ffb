"""The device-resident LaCAM search against its restatement (tests/expert_search_ref.py): status, iterations, nodes, length and
solution of every instance, then actions, planned cells, env positions and done flags after every step of the episode, then logs,
lengths and metrics under tests/test_gpu_expert.py's own metric rules, on the shapes of expert_search_ref.gpu_cases(); launch slices,
a hash cut to one bit, determinism, a clean workspace, the refusals, the evaluation branch and the command-line tool."""
import json
import os

import numpy as np
import pytest

from tests import expert_ref as er
from tests import expert_search_ref as sr
from tests.test_gpu_expert import assert_final_state, smoke_config

pytestmark = pytest.mark.gpu
CASES = sr.gpu_cases()
_REFS = {}


def make_expert(case, **kw):
    import torch
    from mapf_gpt_amd.expert import BatchedExpert
    kw.setdefault("max_iters", case["max_iters"])
    ex = BatchedExpert(case["grids"], case["n_inst"], case["n_agents"], case["steps"], seed=case["seed"], inst_offset=case["inst_offset"],
                       search="lacam", **kw)
    ex.reset(torch.from_numpy(case["pos"]), torch.from_numpy(case["goal"]))
    return ex


def final_ref(name):
    """The restatement after the case's whole episode (computed once, read only)."""
    if name not in _REFS:
        _REFS[name] = sr.run_case(CASES[name])
    return _REFS[name]


def search_bits(ex):
    return [t.cpu().numpy() for t in ex.search_stats()] + [ex.solution().cpu().numpy()]


def assert_search_equals(ex, ref):
    got = search_bits(ex)
    for g, w, what in zip(got, list(ref.stats()) + [ref.solution()], ("status", "iterations", "nodes", "length", "solution")):
        assert np.array_equal(g, w), (what, g.tolist() if g.ndim == 1 else None, w.tolist() if w.ndim == 1 else None)


def episode_bits(ex, steps):
    ex.run(steps)
    log, lens = ex.log()
    return [log.cpu().numpy(), lens.cpu().numpy(), ex.metrics().cpu().numpy(), ex.env.sync_state()[0].cpu().numpy().copy()]


@pytest.mark.parametrize("name", sorted(CASES))
def test_search_and_every_step_equal_the_restatement(name):
    case = CASES[name]
    ex = make_expert(case)
    ref = sr.run_case(case, steps=0)
    assert_search_equals(ex, ref)
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
    whole = dict(er.random_case(12, 12, 0.2, 10, 8, 40, seed=10), max_iters=512)
    assert np.array_equal(whole["pos"][7:], shard["pos"]) and np.array_equal(whole["goal"][7:], shard["goal"])
    a, b = make_expert(whole), make_expert(shard)
    for x, y in zip(search_bits(a), search_bits(b)):
        assert np.array_equal(x[7:], y)
    for x, y in zip(episode_bits(a, 40), episode_bits(b, 40)):
        assert np.array_equal(x[7:], y)
    assert_final_state(b, final_ref("offset7"))


@pytest.mark.parametrize("name,kw", [("grids3", dict(iters_per_launch=7)), ("agents70", dict(iters_per_launch=7)),
                                     ("grids3", dict(hash_bits=1)), ("pocket", dict(hash_bits=1)), ("agents65", dict(hash_bits=1))])
def test_launch_slices_and_a_one_bit_hash_give_the_same_bits(name, kw):
    ex = make_expert(CASES[name], **kw)                         # hash_bits = 1: every lookup walks the table through the equality check
    assert_search_equals(ex, final_ref(name))
    ex.run(CASES[name]["steps"])
    assert_final_state(ex, final_ref(name))


def test_two_runs_give_the_same_bits():
    outs = []
    for _ in range(2):
        ex = make_expert(CASES["agents70"])
        outs.append(search_bits(ex) + episode_bits(ex, CASES["agents70"]["steps"]))
    for x, y in zip(*outs):
        assert np.array_equal(x, y)


def test_reset_searches_again_and_the_workspace_is_left_clean():
    import torch
    from mapf_gpt_amd import _lib
    from tests.test_gpu_expert import make_expert as make_plain
    case = CASES["shared5"]
    ex = make_expert(case)
    ex.run(7)
    ex.reset(torch.from_numpy(case["pos"]), torch.from_numpy(case["goal"]))      # a second episode on the same context
    assert_search_equals(ex, final_ref("shared5"))
    ex.run(case["steps"])
    assert_final_state(ex, final_ref("shared5"))
    assert _lib.lib().mgpt_expert_set_search(ex._h, 16, 0, 0) == _lib.OK         # set_search may be called again
    for name in ("shared5", "agents70", "pocket"):              # solved, out of iterations, open ran empty
        srch = make_expert(CASES[name])
        plain = make_plain(dict(CASES[name]))                   # a plain expert built after a search-mode one on the same shapes
        plain.run(CASES[name]["steps"])
        assert_final_state(plain, er.run_case(CASES[name]))
        del srch


def test_argument_and_state_refusals():
    import torch
    from mapf_gpt_amd import _lib
    from mapf_gpt_amd.expert import BatchedExpert
    case = CASES["swap2"]
    L = _lib.lib()
    with pytest.raises(ValueError):
        BatchedExpert(case["grids"], 1, 2, 8, search="cbs")
    ex = BatchedExpert(case["grids"], 1, 2, 16)
    assert L.mgpt_expert_set_search(None, 8, 0, 0) == _lib.ERR_ARG
    for bad in [(0, 0, 0), (-1, 0, 0), ((1 << 24) + 1, 0, 0), (8, -1, 0), (8, 0, -1), (8, 0, 64)]:
        assert L.mgpt_expert_set_search(ex._h, *bad) == _lib.ERR_ARG, bad
    assert L.mgpt_expert_solve(None, None) == _lib.ERR_ARG
    assert L.mgpt_expert_solve(ex._h, None) == _lib.ERR_STATE and b"set_search" in L.mgpt_last_error()
    out = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert L.mgpt_expert_copy_search(ex._h, _lib.ptr(out), None, None, None, None) == _lib.ERR_STATE
    assert L.mgpt_expert_set_search(ex._h, 64, 0, 0) == _lib.OK
    assert L.mgpt_expert_solve(ex._h, None) == _lib.ERR_STATE and b"reset" in L.mgpt_last_error()      # solve before reset
    ex.env.reset(torch.from_numpy(case["pos"]), torch.from_numpy(case["goal"]))
    ex.tok.create_agents(ex.env.pos, ex.env.goal)
    assert L.mgpt_expert_reset(ex._h, None) == _lib.OK
    with pytest.raises(_lib.MGPTError) as e:                    # search mode: step before solve
        ex.step()
    assert e.value.code == _lib.ERR_STATE
    assert L.mgpt_expert_copy_solution(ex._h, None, None) == _lib.ERR_ARG
    sol = torch.zeros((1, 2, 16), dtype=torch.int8, device="cuda")
    assert L.mgpt_expert_copy_solution(ex._h, _lib.ptr(sol), None) == _lib.ERR_STATE
    assert L.mgpt_expert_solve(ex._h, None) == _lib.OK
    assert L.mgpt_expert_copy_search(ex._h, _lib.ptr(out), None, None, None, None) == _lib.OK
    torch.cuda.synchronize()
    assert out.item() == 1
    ex.step()
    assert L.mgpt_expert_solve(ex._h, None) == _lib.ERR_STATE   # not in the middle of an episode
    plain = BatchedExpert(case["grids"], 1, 2, 16)              # without set_search nothing changes
    plain.reset(torch.from_numpy(case["pos"]), torch.from_numpy(case["goal"]))
    with pytest.raises(_lib.MGPTError):
        plain.search_stats()


def lacam_config():
    cfg = smoke_config()
    del cfg["algorithms"]["MAPF-GPT-2M"]
    cfg["algorithms"]["LaCAM"] = {"name": "LaCAM", "seed": 0, "max_iters": 256}
    cfg["environment"]["num_agents"] = 8
    return cfg


def test_evaluation_runs_a_lacam_algorithm(tmp_path):
    from mapf_gpt_amd import evaluation as ev
    status = {}
    res = ev.evaluation(lacam_config(), eval_dir=str(tmp_path), print_fn=lambda *_: None, log_actions=True, search_status=status)
    assert len(res) == 16 and os.path.exists(tmp_path / "PIBT.json") and os.path.exists(tmp_path / "LaCAM.json")
    assert sum(status.values()) == 8 and set(status) <= {1, 2, 3, 4}
    pibt = {json.dumps(r["env_grid_search"], sort_keys=True): r for r in res if r["algorithm"] == "PIBT"}
    lacam = [r for r in res if r["algorithm"] == "LaCAM"]
    assert len(lacam) == 8
    for r in lacam:
        m, p = r["metrics"], pibt[json.dumps(r["env_grid_search"], sort_keys=True)]["metrics"]
        assert set(m) == set(p) and len(m["made_actions"]) == 8 and all(len(a) == int(m["ep_length"]) for a in m["made_actions"])
        assert m["CSR"] >= p["CSR"]                             # a fallback episode IS the PIBT episode, a replayed one is solved
        if m["CSR"] < 1:
            assert m["made_actions"] == p["made_actions"]
    with pytest.raises(TypeError):
        ev.LaCAMConfig(name="LaCAM", batch_size=4)              # unknown keys raise


def test_cli_lacam_log_round_trips_through_split_by_map_and_the_tokenizer(tmp_path, capfd):
    import yaml
    from mapf_gpt_amd import dataset_build, dataset_tokenizer as dt, expert, maps
    cfg = lacam_config()
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    assert expert.main(["--config", str(tmp_path / "cfg.yaml"), "--out", str(tmp_path / "out"), "--algo", "lacam", "--max-iters", "256"]) == 0
    line = json.loads(capfd.readouterr().out.strip().splitlines()[-1])
    assert set(line) == {"episodes", "solved", "rows", "seconds", "status"} and line["episodes"] == 8
    assert sum(line["status"].values()) == 8 and line["solved"] >= line["status"].get("1", 0)
    assert not os.path.exists(tmp_path / "out" / "PIBT.json")
    per_map = dataset_build.split_by_map(str(tmp_path / "out" / "LaCAM.json"), str(tmp_path / "temp"))
    res = [r for v in per_map.values() for r in v]
    assert len(res) == 8 and all(r["algorithm"] == "LaCAM" for r in res)
    assert line["solved"] == sum(r["metrics"]["CSR"] >= 1 for r in res)
    named = {k: "\n".join(v) for k, v in maps.named_maps().items() if k.startswith("validation-")}
    inputs, labels = dt.ObservationGenerator(named, res).generate_observations(0, len(res))
    assert line["solved"] > 0 and len(inputs) == len(labels) == line["rows"]
