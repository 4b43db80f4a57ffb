"""The corridor swap rule on the device against its restatement (tests/expert_swap_ref.py), case by case under
tests/test_gpu_expert.py's metric rules: actions, planned cells, env positions and done flags after every step, logs, lengths and
metrics at the end, and in search mode status, iterations, nodes, length and solution; shards, launch slices, a hash cut to one bit,
determinism, the switch turned off again, the refusals, the evaluation branch and the command-line tool.  No share of solved episodes
is asserted here."""
import json
import os

import numpy as np
import pytest

from tests import expert_ref as er
from tests import expert_search_ref as sr
from tests import expert_swap_ref as sw
from tests.test_gpu_expert import assert_final_state, smoke_config
from tests.test_gpu_expert_search import assert_search_equals, episode_bits, search_bits

pytestmark = pytest.mark.gpu
CASES = sw.gpu_cases()
_REFS = {}


def make_expert(case, search=False, **kw):
    import torch
    from mapf_gpt_amd.expert import BatchedExpert
    if search:
        kw.update(search="lacam")
        kw.setdefault("max_iters", case["max_iters"])
    kw.setdefault("swap", True)
    ex = BatchedExpert(case["grids"], case["n_inst"], case["n_agents"], case["steps"], seed=case["seed"], inst_offset=case["inst_offset"], **kw)
    ex.reset(torch.from_numpy(case["pos"]), torch.from_numpy(case["goal"]))
    return ex


def final_ref(name, search=False):
    """The restatement after the case's whole episode (computed once, read only)."""
    if (name, search) not in _REFS:
        _REFS[name, search] = (sw.run_search_case if search else sw.run_case)(CASES[name])
    return _REFS[name, search]


def assert_every_step_equals(ex, ref, steps):
    for t in range(steps):
        ex.step()
        act, planned = ref.step()
        pos, _, done = ex.env.sync_state()
        assert np.array_equal(ex.actions.cpu().numpy(), act), f"actions differ at step {t}"
        assert np.array_equal(ex.planned().cpu().numpy(), planned), f"planned cells differ at step {t}"
        assert np.array_equal(pos.cpu().numpy(), ref.pos), f"env positions differ at step {t}"
        assert np.array_equal(done.cpu().numpy(), ref.done), f"done flags differ at step {t}"
    assert_final_state(ex, ref)


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_step_equals_the_restatement(name):
    case = CASES[name]
    assert_every_step_equals(make_expert(case), sw.run_case(case, steps=0), case["steps"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_search_and_every_step_equal_the_restatement(name):
    case = CASES[name]
    ex = make_expert(case, search=True)
    ref = sw.run_search_case(case, steps=0)
    assert_search_equals(ex, ref)
    assert_every_step_equals(ex, ref, case["steps"])


def test_a_shard_equals_the_same_instances_of_the_unsharded_run():
    shard = CASES["offset7"]
    whole = dict(er.random_case(12, 12, 0.2, 10, 8, 40, seed=10), max_iters=sw.MAX_ITERS)
    assert np.array_equal(whole["pos"][7:], shard["pos"]) and np.array_equal(whole["goal"][7:], shard["goal"])
    for search in (False, True):
        a, b = make_expert(whole, search), make_expert(shard, search)
        if search:
            for x, y in zip(search_bits(a), search_bits(b)):
                assert np.array_equal(x[7:], y)
        for x, y in zip(episode_bits(a, 40), episode_bits(b, 40)):
            assert np.array_equal(x[7:], y)
        assert_final_state(b, final_ref("offset7", search))


@pytest.mark.parametrize("name,kw", [("maze16", dict(iters_per_launch=7)), ("agents70", dict(iters_per_launch=7)),
                                     ("maze16", dict(hash_bits=1)), ("swap3", dict(hash_bits=1)), ("rests3", dict(iters_per_launch=7))])
def test_launch_slices_and_a_one_bit_hash_give_the_same_bits(name, kw):
    ex = make_expert(CASES[name], search=True, **kw)
    assert_search_equals(ex, final_ref(name, True))
    ex.run(CASES[name]["steps"])
    assert_final_state(ex, final_ref(name, True))


@pytest.mark.parametrize("name", ["agents70", "maze16"])
def test_two_runs_give_the_same_bits(name):
    outs = []
    for _ in range(2):
        ex = make_expert(CASES[name], search=True)
        outs.append(search_bits(ex) + episode_bits(ex, CASES[name]["steps"]))
        plain = make_expert(CASES[name])
        outs[-1] += episode_bits(plain, CASES[name]["steps"])
    for x, y in zip(*outs):
        assert np.array_equal(x, y)


def test_the_switch_turned_off_again_gives_the_plain_experts_bits():
    import torch
    from tests.test_gpu_expert import make_expert as make_plain
    for name in ("swap3", "maze16"):
        case = CASES[name]
        pos, goal = torch.from_numpy(case["pos"]), torch.from_numpy(case["goal"])
        ex = make_expert(case)
        ex.run(case["steps"])                                   # a swap episode, to its end
        assert_final_state(ex, final_ref(name))
        ex.set_swap(False)
        ex.reset(pos, goal)
        ex.run(case["steps"])
        assert_final_state(ex, er.run_case(case))
        ex.set_swap(True)                                       # and on again: the degree map is still there
        ex.reset(pos, goal)
        ex.run(case["steps"])
        assert_final_state(ex, final_ref(name))
        srch = make_expert(case, search=True)                   # search mode: off again gives expert_search_ref's bits
        srch.run(case["steps"])
        srch.set_swap(False)
        srch.reset(pos, goal)
        want = sr.run_case(case, max_iters=case["max_iters"])
        assert_search_equals(srch, want)
        srch.run(case["steps"])
        assert_final_state(srch, want)
        plain = make_plain(dict(case))                          # a plain expert built afterwards on the same shapes
        plain.run(case["steps"])
        assert_final_state(plain, er.run_case(case))


def test_set_search_and_set_swap_in_either_order():
    import torch
    from mapf_gpt_amd import _lib
    from mapf_gpt_amd.expert import BatchedExpert
    case = CASES["swap3"]
    ex = BatchedExpert(case["grids"], 1, 3, case["steps"], seed=case["seed"])
    assert _lib.lib().mgpt_expert_set_swap(ex._h, 1) == _lib.OK
    assert _lib.lib().mgpt_expert_set_search(ex._h, case["max_iters"], 0, 0) == _lib.OK
    ex.search, ex.max_iters = "lacam", case["max_iters"]
    ex.reset(torch.from_numpy(case["pos"]), torch.from_numpy(case["goal"]))
    assert_search_equals(ex, final_ref("swap3", True))
    ex.run(case["steps"])
    assert_final_state(ex, final_ref("swap3", True))


def test_argument_and_state_refusals():
    import torch
    from mapf_gpt_amd import _lib
    from mapf_gpt_amd.expert import BatchedExpert
    case = CASES["swap2"]
    L = _lib.lib()
    pos, goal = torch.from_numpy(case["pos"]), torch.from_numpy(case["goal"])
    ex = BatchedExpert(case["grids"], 1, 2, 16, seed=case["seed"])
    assert L.mgpt_expert_set_swap(None, 1) == _lib.ERR_ARG
    for bad in (2, -1, 256):
        assert L.mgpt_expert_set_swap(ex._h, bad) == _lib.ERR_ARG, bad
    assert L.mgpt_expert_set_swap(ex._h, 1) == _lib.OK and L.mgpt_expert_set_swap(ex._h, 0) == _lib.OK      # before reset
    ex.reset(pos, goal)
    assert L.mgpt_expert_set_swap(ex._h, 1) == _lib.OK          # right after reset nothing has been planned yet
    ex.step()
    assert L.mgpt_expert_set_swap(ex._h, 0) == _lib.ERR_STATE and b"episode" in L.mgpt_last_error()
    assert L.mgpt_expert_set_swap(ex._h, 1) == _lib.ERR_STATE   # the value does not matter
    assert L.mgpt_expert_set_swap(ex._h, 2) == _lib.ERR_ARG     # the argument is looked at first
    with pytest.raises(_lib.MGPTError) as e:
        ex.set_swap(False)
    assert e.value.code == _lib.ERR_STATE
    ex.run(15)                                                  # with the rule the episode ends solved after 6 steps
    assert ex.metrics()[0, 0].item() == 1.0 and ex.metrics()[0, 4].item() == 6
    assert L.mgpt_expert_set_swap(ex._h, 0) == _lib.OK          # between episodes
    srch = BatchedExpert(case["grids"], 1, 2, 16, seed=case["seed"], search="lacam", max_iters=64)
    srch.reset(pos, goal)                                       # reset solves: the episode has begun
    assert L.mgpt_expert_set_swap(srch._h, 1) == _lib.ERR_STATE


def swap_config(lacam=True):
    cfg = smoke_config()
    del cfg["algorithms"]["MAPF-GPT-2M"]
    cfg["algorithms"]["PIBT"] = {"name": "PIBT", "seed": 0, "swap": True}
    if lacam:
        cfg["algorithms"]["LaCAM"] = {"name": "LaCAM", "seed": 0, "max_iters": 256, "swap": True}
    cfg["environment"]["num_agents"] = 8
    return cfg


def test_evaluation_runs_swap_entries_and_the_tokenizer_takes_their_records(tmp_path):
    from mapf_gpt_amd import dataset_tokenizer as dt, evaluation as ev, maps
    status = {}
    res = ev.evaluation(swap_config(), eval_dir=str(tmp_path), print_fn=lambda *_: None, log_actions=True, search_status=status)
    assert len(res) == 16 and os.path.exists(tmp_path / "PIBT.json") and os.path.exists(tmp_path / "LaCAM.json")
    assert sum(status.values()) == 8 and set(status) <= {1, 2, 3, 4}
    for r in res:
        m = r["metrics"]
        assert len(m["made_actions"]) == 8 and all(len(a) == int(m["ep_length"]) for a in m["made_actions"])
    named = {k: "\n".join(v) for k, v in maps.named_maps().items() if k.startswith("validation-")}
    inputs, labels = dt.ObservationGenerator(named, res).generate_observations(0, len(res))
    assert len(inputs) == len(labels) == sum(8 * (int(r["metrics"]["ep_length"]) + 1) for r in res if r["metrics"]["CSR"] >= 1)
    c = ev.PIBTConfig(name="PIBT")
    assert c.swap is False and ev.LaCAMConfig(name="LaCAM", swap=True).swap is True
    with pytest.raises(TypeError):
        ev.PIBTConfig(name="PIBT", swap=True, batch_size=4)     # unknown keys still raise


@pytest.mark.parametrize("algo", ["pibt", "lacam"])
def test_cli_swap_log_round_trips_through_split_by_map_and_the_tokenizer(tmp_path, capfd, algo):
    import yaml
    from mapf_gpt_amd import dataset_build, dataset_tokenizer as dt, expert, maps
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(swap_config(lacam=False), f)
    argv = ["--config", str(tmp_path / "cfg.yaml"), "--out", str(tmp_path / "out"), "--swap"]
    fname = "PIBT.json"
    if algo == "lacam":
        argv, fname = argv + ["--algo", "lacam", "--max-iters", "256"], "LaCAM.json"
    assert expert.main(argv) == 0
    line = json.loads(capfd.readouterr().out.strip().splitlines()[-1])
    assert set(line) == {"episodes", "solved", "rows", "seconds", "swap"} | ({"status"} if algo == "lacam" else set())
    assert line["swap"] is True and line["episodes"] == 8
    other = "LaCAM.json" if fname == "PIBT.json" else "PIBT.json"
    assert os.path.exists(tmp_path / "out" / fname) and not os.path.exists(tmp_path / "out" / other)      # the file names do not change
    per_map = dataset_build.split_by_map(str(tmp_path / "out" / fname), str(tmp_path / "temp"))
    res = [r for v in per_map.values() for r in v]
    assert len(res) == 8 and line["solved"] == sum(r["metrics"]["CSR"] >= 1 for r in res)
    named = {k: "\n".join(v) for k, v in maps.named_maps().items() if k.startswith("validation-")}
    inputs, labels = dt.ObservationGenerator(named, res).generate_observations(0, len(res))
    assert len(inputs) == len(labels) == line["rows"]
