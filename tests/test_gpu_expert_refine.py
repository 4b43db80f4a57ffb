"""The refinement pass on the device against its restatement (tests/expert_refine_ref.py), case by case with the
swap rule off and on: final status and length, first status and length, SoC before and after, rounds and replans, the solution, then
actions, planned cells, env positions and done flags after every step (each step also through expert_checks.check_transition), then
logs, lengths and metrics under tests/test_gpu_expert.py's metric rules; one round only, a horizon that leaves an instance out, shards,
determinism, a second reset, the pass turned off, the refusals, the evaluation branch and the command-line tool.  No share of solved
or rescued episodes is asserted here."""
import json
import os

import numpy as np
import pytest

from tests import expert_checks as ck
from tests import expert_ref as er
from tests import expert_refine_ref as rr
from tests.test_gpu_expert import assert_final_state, smoke_config
from tests.test_gpu_expert_search import episode_bits, search_bits

pytestmark = pytest.mark.gpu
CASES = rr.gpu_cases()
_REFS = {}


def make_expert(case, swap=False, rounds=rr.ROUNDS, **kw):
    import torch
    from mapf_gpt_amd.expert import BatchedExpert
    kw.setdefault("max_iters", case["max_iters"])
    ex = BatchedExpert(case["grids"], case["n_inst"], case["n_agents"], case["steps"], seed=case["seed"], inst_offset=case["inst_offset"],
                       search="lacam", swap=swap, refine_rounds=rounds, **kw)
    ex.reset(torch.from_numpy(case["pos"]), torch.from_numpy(case["goal"]))
    return ex


def final_ref(name, swap=False, **kw):
    """The restatement after the case's whole episode (computed once, read only)."""
    key = (name, swap, tuple(sorted(kw.items())))
    if key not in _REFS:
        _REFS[key] = rr.run_case(CASES[name], swap=swap, **kw)
    return _REFS[key]


def refine_bits(ex):
    return search_bits(ex) + [t.cpu().numpy() for t in ex.refine_stats()]


def assert_refine_equals(ex, ref):
    status, iters, nodes, length = ref.stats()
    got_status, got_iters, got_nodes, got_length = (t.cpu().numpy() for t in ex.search_stats())
    assert np.array_equal(got_status, status), ("final status", got_status.tolist(), status.tolist())
    assert np.array_equal(got_length, length), ("final length", got_length.tolist(), length.tolist())
    for g, w, what in zip(ex.refine_stats(), ref.refine_stats(), ("first status", "first length", "SoC before", "SoC after", "rounds", "replans")):
        assert np.array_equal(g.cpu().numpy(), w), (what, g.cpu().tolist(), w.tolist())
    assert np.array_equal(ex.solution().cpu().numpy(), ref.solution()), "solution"
    assert np.array_equal(got_iters, iters) and np.array_equal(got_nodes, nodes)         # the search's own, unchanged


def assert_every_step_equals(ex, ref, case):
    grids = case["grids"]
    for t in range(case["steps"]):
        before, _, skip = (x.cpu().numpy().copy() for x in ex.env.sync_state())
        ex.step()
        act, planned = ref.step()
        pos, _, done = ex.env.sync_state()
        got_act, got_planned = ex.actions.cpu().numpy(), ex.planned().cpu().numpy()
        ck.check_transition(grids, before, got_act, got_planned, pos.cpu().numpy(), skip != 0)
        assert np.array_equal(got_act, act), f"actions differ at step {t}"
        assert np.array_equal(got_planned, planned), f"planned cells differ at step {t}"
        assert np.array_equal(pos.cpu().numpy(), ref.pos), f"env positions differ at step {t}"
        assert np.array_equal(done.cpu().numpy(), ref.done), f"done flags differ at step {t}"
    assert_final_state(ex, ref)


@pytest.mark.parametrize("swap", [False, True], ids=["plain", "swap"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_refinement_and_every_step_equal_the_restatement(name, swap):
    case = CASES[name]
    ex = make_expert(case, swap)
    ref = rr.run_case(case, steps=0, swap=swap)
    assert_refine_equals(ex, ref)
    assert_every_step_equals(ex, ref, case)


@pytest.mark.parametrize("name,swap,kw", [("offset7", False, dict(max_rounds=1)), ("swap2", False, dict(max_rounds=1)),
                                          ("agents65", True, dict(max_rounds=1)), ("grids3", False, dict(horizon=40)),
                                          ("offset7", False, dict(horizon=58))])
def test_one_round_only_and_a_horizon_that_leaves_an_instance_out(name, swap, kw):
    case = CASES[name]
    ex = make_expert(case, swap, rounds=kw.get("max_rounds", rr.ROUNDS), refine_horizon=kw.get("horizon"))
    ref = final_ref(name, swap, **kw)
    assert_refine_equals(ex, ref)
    first, _, _, _, rounds, replans = ref.refine_stats()
    if "horizon" in kw:                                         # instance 0 is longer than the horizon: untouched, its neighbours refined
        assert ref.stats()[0][0] == 4 and rounds[0] == 0 and (rounds[1:] > 0).all()
    else:                                                       # a second round would adopt more
        assert (rounds <= 1).all() and replans.sum() < final_ref(name, swap).refine_stats()[5].sum()
    ex.run(case["steps"])
    assert_final_state(ex, ref)


def test_a_map_whose_layers_need_more_than_64_kb_of_lds():
    case = dict(er.random_case(40, 40, 0.2, 2, 8, 128, seed=12), max_iters=512)      # 50 x 50 cells: 257 layers of 314 bytes
    ex = make_expert(case)
    ref = rr.run_case(case, steps=0)
    assert ref.refine_stats()[5].sum() > 0
    assert_refine_equals(ex, ref)
    ex.run(64)
    ref.run(64)
    assert_final_state(ex, ref)


@pytest.mark.parametrize("swap", [False, True], ids=["plain", "swap"])
def test_a_shard_equals_the_same_instances_of_the_unsharded_run(swap):
    shard = CASES["offset7"]
    whole = dict(er.random_case(12, 12, 0.2, 10, 8, 40, seed=10), max_iters=shard["max_iters"])
    assert np.array_equal(whole["pos"][7:], shard["pos"]) and np.array_equal(whole["goal"][7:], shard["goal"])
    a, b = make_expert(whole, swap), make_expert(shard, swap)
    for x, y in zip(refine_bits(a), refine_bits(b)):
        assert np.array_equal(x[7:], y)
    for x, y in zip(episode_bits(a, 40), episode_bits(b, 40)):
        assert np.array_equal(x[7:], y)
    assert_final_state(b, final_ref("offset7", swap))


@pytest.mark.parametrize("name,swap", [("agents65", False), ("agents70", True)])
def test_two_runs_give_the_same_bits(name, swap):
    outs = []
    for _ in range(2):
        ex = make_expert(CASES[name], swap)
        outs.append(refine_bits(ex) + episode_bits(ex, CASES[name]["steps"]))
    for x, y in zip(*outs):
        assert np.array_equal(x, y)


def test_a_second_reset_refines_again_and_the_pass_off_is_the_plain_search():
    import torch
    from tests.test_gpu_expert import make_expert as make_plain
    from tests.test_gpu_expert_search import make_expert as make_search
    for name in ("shared5", "grids3"):
        case = CASES[name]
        pos, goal = torch.from_numpy(case["pos"]), torch.from_numpy(case["goal"])
        ex = make_expert(case)
        ex.run(7)
        ex.reset(pos, goal)                                     # a second episode on the same context
        assert_refine_equals(ex, final_ref(name))
        ex.run(case["steps"])
        assert_final_state(ex, final_ref(name))
        ex.set_refine(0)                                        # between episodes: off again gives the plain search-mode expert's bits
        ex.reset(pos, goal)
        off, zero, plain = search_bits(ex), make_expert(case, rounds=0), make_search(case)
        for x, y, z in zip(off + episode_bits(ex, case["steps"]), search_bits(zero) + episode_bits(zero, case["steps"]),
                           search_bits(plain) + episode_bits(plain, case["steps"])):
            assert np.array_equal(x, z) and np.array_equal(y, z)
        pibt = make_plain(dict(case))                           # a plain expert built afterwards on the same shapes
        pibt.run(case["steps"])
        assert_final_state(pibt, er.run_case(case))


def test_argument_and_state_refusals():
    import torch
    from mapf_gpt_amd import _lib
    from mapf_gpt_amd.expert import BatchedExpert
    case = CASES["swap2"]
    L = _lib.lib()
    pos, goal = torch.from_numpy(case["pos"]), torch.from_numpy(case["goal"])
    with pytest.raises(ValueError):
        BatchedExpert(case["grids"], 1, 2, 16, refine_rounds=4)                  # needs search="lacam"
    ex = BatchedExpert(case["grids"], 1, 2, 16, seed=case["seed"])
    assert L.mgpt_expert_set_refine(None, 4, 0) == _lib.ERR_ARG
    assert L.mgpt_expert_set_refine(ex._h, 4, 0) == _lib.ERR_STATE and b"set_search" in L.mgpt_last_error()
    assert L.mgpt_expert_set_search(ex._h, 64, 0, 0) == _lib.OK
    for bad in [(-1, 0), ((1 << 16) + 1, 0), (4, -1), (4, 15), (4, (1 << 20) + 1)]:
        assert L.mgpt_expert_set_refine(ex._h, *bad) == _lib.ERR_ARG, bad
    out = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(6)]
    ptrs = [_lib.ptr(t) for t in out]
    assert L.mgpt_expert_copy_refine(None, *ptrs, None) == _lib.ERR_ARG
    assert L.mgpt_expert_copy_refine(ex._h, *ptrs, None) == _lib.ERR_STATE       # the pass is off
    assert L.mgpt_expert_set_refine(ex._h, 4, 16) == _lib.OK and L.mgpt_expert_set_refine(ex._h, 0, 0) == _lib.OK
    ex.search = "lacam"
    ex.reset(pos, goal)                                         # solves
    assert L.mgpt_expert_copy_refine(ex._h, *ptrs, None) == _lib.ERR_STATE       # solved, but the pass is off
    assert L.mgpt_expert_set_refine(ex._h, 4, 0) == _lib.ERR_STATE and b"episode" in L.mgpt_last_error()
    ex.run(16)                                                  # the search's 9 steps end the episode
    assert L.mgpt_expert_set_refine(ex._h, 4, 0) == _lib.OK     # between episodes
    assert L.mgpt_expert_copy_refine(ex._h, *ptrs, None) == _lib.ERR_STATE       # on, but not solved yet
    ex.reset(pos, goal)
    assert L.mgpt_expert_copy_refine(ex._h, *ptrs[:2], None, None, None, ptrs[5], None) == _lib.OK        # any may be NULL
    torch.cuda.synchronize()
    assert [t.item() for t in out] == [1, 9, 0, 0, 0, 4]
    ex.step()
    with pytest.raises(_lib.MGPTError) as e:
        ex.set_refine(0)
    assert e.value.code == _lib.ERR_STATE
    assert L.mgpt_expert_set_search(ex._h, 64, 0, 0) == _lib.OK                  # set_search again turns the pass off
    assert L.mgpt_expert_copy_refine(ex._h, *ptrs, None) == _lib.ERR_STATE
    big = BatchedExpert(np.zeros((1, 96, 96), np.uint8), 1, 2, 64, search="lacam", max_iters=4)
    assert L.mgpt_expert_set_refine(big._h, 4, 0) == _lib.ERR_UNSUPPORTED and b"96 x 96" in L.mgpt_last_error()      # 129 layers of 1152 bytes
    assert L.mgpt_expert_set_refine(big._h, 4, 64) == _lib.OK and L.mgpt_expert_set_refine(big._h, 0, 0) == _lib.OK  # 65 layers fit


def refine_config(rounds=8):
    cfg = smoke_config()
    del cfg["algorithms"]["MAPF-GPT-2M"], cfg["algorithms"]["PIBT"]
    cfg["algorithms"]["LaCAM"] = {"name": "LaCAM", "seed": 0, "max_iters": 256}
    cfg["algorithms"]["LaCAM-refined"] = {"name": "LaCAM", "seed": 0, "max_iters": 256, "refine_rounds": rounds}
    cfg["environment"]["num_agents"] = 8
    return cfg


def test_evaluation_with_refine_rounds_is_never_worse_than_the_plain_entry(tmp_path):
    from mapf_gpt_amd import evaluation as ev
    stats, status = {}, {}
    cfg = refine_config()
    plain_only = dict(cfg, algorithms={"LaCAM": cfg["algorithms"]["LaCAM"]})
    ev.evaluation(plain_only, eval_dir=str(tmp_path / "plain"), print_fn=lambda *_: None, search_status=status)
    res = ev.evaluation(cfg, eval_dir=str(tmp_path), print_fn=lambda *_: None, log_actions=True, refine_stats=stats)
    plain = {json.dumps(r["env_grid_search"], sort_keys=True): r["metrics"] for r in res if r["algorithm"] == "LaCAM"}
    fine = {json.dumps(r["env_grid_search"], sort_keys=True): r["metrics"] for r in res if r["algorithm"] == "LaCAM-refined"}
    assert len(plain) == len(fine) == 8 and set(plain) == set(fine)
    assert set(stats) == {"refined", "rescued", "soc_before", "soc_after"} and stats["soc_after"] <= stats["soc_before"]
    assert sum(m["CSR"] >= 1 for m in fine.values()) >= sum(m["CSR"] >= 1 for m in plain.values())
    longer = 0
    for k, m in fine.items():
        p = plain[k]
        assert m["CSR"] >= p["CSR"]
        if p["CSR"] >= 1 and m["CSR"] >= 1:
            longer += m["ep_length"] > p["ep_length"]
        if m["CSR"] < 1:                                        # both fall back: the PIBT episode
            assert m["made_actions"] == p["made_actions"]
    # a status-1 instance is replayed by both entries, the refined one no longer; a status-2 or -3 instance falls back in both, the same
    # episode; only an instance the plain search left over the cap (status 4: PIBT's episode there, a replay here) may come out longer
    assert longer <= status.get(4, 0)
    c = ev.LaCAMConfig(name="LaCAM")
    assert c.refine_rounds == 0 and c.refine_horizon is None and ev.LaCAMConfig(name="LaCAM", refine_rounds=3, refine_horizon=64).refine_horizon == 64
    with pytest.raises(TypeError):
        ev.PIBTConfig(name="PIBT", refine_rounds=3)             # the plain PIBT expert has no solution to refine


def test_cli_refined_log_round_trips_through_split_by_map_and_the_tokenizer(tmp_path, capfd):
    import yaml
    from mapf_gpt_amd import dataset_build, dataset_tokenizer as dt, expert, maps
    cfg = refine_config()
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    assert expert.main(["--config", str(tmp_path / "cfg.yaml"), "--out", str(tmp_path / "out"), "--algo", "lacam", "--max-iters", "256",
                        "--refine-rounds", "8"]) == 0
    line = json.loads(capfd.readouterr().out.strip().splitlines()[-1])
    assert set(line) == {"episodes", "solved", "rows", "seconds", "status", "refine_rounds", "refined", "rescued", "soc_before", "soc_after"}
    assert line["episodes"] == 8 and line["refine_rounds"] == 8 and line["soc_after"] <= line["soc_before"]
    assert 0 <= line["rescued"] <= line["refined"] <= 8
    assert os.path.exists(tmp_path / "out" / "LaCAM.json") and not os.path.exists(tmp_path / "out" / "PIBT.json")   # the file names do not change
    per_map = dataset_build.split_by_map(str(tmp_path / "out" / "LaCAM.json"), str(tmp_path / "temp"))
    res = [r for v in per_map.values() for r in v]
    assert len(res) == 8 and line["solved"] == sum(r["metrics"]["CSR"] >= 1 for r in res)
    named = {k: "\n".join(v) for k, v in maps.named_maps().items() if k.startswith("validation-")}
    inputs, labels = dt.ObservationGenerator(named, res).generate_observations(0, len(res))
    assert line["solved"] > 0 and len(inputs) == len(labels) == line["rows"]
