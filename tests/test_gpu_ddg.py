"""Delta data generation on the device against its restatement (tests/ddg_ref.py): the hand trajectory, the tiny
policy's own recorded episode stage by stage, chunking, determinism, the lifelong refusal and the CLI's log through the dataset path."""
import json
import os

import numpy as np
import pytest

from tests import ddg_ref as dr
from tests import expert_ref as er

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = ("valid", "solved", "cost", "picked", "j", "dmax")
_cache = {}


def assert_same(got, want):
    for k in TABLES:
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    assert got["probed"] == want["probed"]
    assert np.array_equal(got["teacher_metrics"][:, :5], want["teacher_metrics"][:, :5].astype(np.float32))
    # avg_agents_density: a float64 mean rounded to float32 on the device, the same terms summed in another order in the restatement:
    # at most one unit in the last place apart (tests/test_gpu_expert.py)
    assert np.allclose(got["teacher_metrics"][:, 5], want["teacher_metrics"][:, 5].astype(np.float32), rtol=2.0 ** -23, atol=0)
    assert len(got["records"]) == len(want["records"]) == int(want["picked"].sum())
    for a, b in zip(got["records"], want["records"]):
        assert a["algorithm"] == b["algorithm"] == "DDG" and a["env_grid_search"] == b["env_grid_search"]
        assert set(a["metrics"]) == set(b["metrics"])
        for k in ("CSR", "ISR", "SoC", "makespan", "ep_length"):
            assert a["metrics"][k] == float(np.float32(b["metrics"][k])), k
        for k in ("made_actions", "init_positions"):
            assert a["metrics"][k] == b["metrics"][k], k


def assert_same_bits(a, b):
    for k in TABLES + ("delta", "cand", "teacher_metrics"):
        assert np.array_equal(a[k], b[k]), k
    assert a["records"] == b["records"] and a["probed"] == b["probed"]


@pytest.mark.parametrize("probe", [dict(), dict(swap=True)], ids=["pibt", "pibt_swap"])
def test_the_hand_trajectory_picks_the_third_segment(probe):
    from mapf_gpt_amd import ddg
    h = dr.hand_trajectory()
    args = (h["grids"], h["pos_traj"], h["lengths"], h["goal"], h["run_keys"])
    got = ddg.collect_from_trajectory(*args, every=h["every"], probe=probe)
    want = dr.collect(*args, h["every"], probe, ddg.TEACHER)
    assert got["picked"].tolist() == [True] and got["j"].tolist() == [2] and got["records"][0]["env_grid_search"]["ddg_step"] == 8
    assert got["solved"].all() and got["records"][0]["metrics"]["CSR"] == 1.0
    assert_same(got, want)


def _policy_run():
    """The tiny policy's recorded episode on dr.POLICY_CASE and everything collect() makes of it, once."""
    if not _cache:
        import torch
        from mapf_gpt_amd import ddg
        from mapf_gpt_amd.model import build_model
        from mapf_gpt_amd.runner import BatchedRunner
        c = dr.POLICY_CASE
        case = er.random_case(c["h"], c["w"], c["density"], c["n_inst"], c["n_agents"], c["T"], seed=c["seed"], map_seed=c["map_seed"])
        net = build_model("tiny", seed=0, max_rows=64, precision="f32")
        run = BatchedRunner(case["grids"], c["n_inst"], c["n_agents"], net, max_episode_steps=c["T"], seed=c["seed"], do_sample=True,
                            precision="f32", record=True)
        run.reset(torch.from_numpy(case["pos"]), torch.from_numpy(case["goal"]))
        run.run(c["T"])
        keys = [{"map_name": "random10", "seed": i, "num_agents": c["n_agents"]} for i in range(c["n_inst"])]
        kw = dict(every=c["every"], teacher=dict(ddg.TEACHER, max_iters=256), seed=c["seed"], global_ids=[3, 4, 5, 9])
        _cache.update(case=case, run=run, keys=keys, kw=kw, out=ddg.collect(run, case["grids"], case["goal"], keys, **kw))
    return _cache


def test_collect_behind_the_tiny_policy_equals_the_restatement_stage_by_stage():
    from mapf_gpt_amd import ddg
    C = _policy_run()
    pos, _, lengths = (x.cpu().numpy() for x in C["run"].trajectory())
    kw = dict(C["kw"])
    want = dr.collect(C["case"]["grids"], pos, lengths, C["case"]["goal"], C["keys"], kw.pop("every"), ddg.PROBE, kw.pop("teacher"),
                      max_episode_steps=dr.POLICY_CASE["T"], **kw)
    got = C["out"]
    assert got["picked"].sum() >= 1, "no instance was picked: the comparison would be between empty lists"
    assert sum(r["metrics"]["CSR"] >= 1 for r in got["records"]) >= 1, "no teacher episode was solved"
    assert_same(got, want)
    for r, i in zip(got["records"], np.nonzero(got["picked"])[0]):
        assert r["metrics"]["init_positions"] == pos[int(got["j"][i]) * 8, i].tolist()
        assert r["env_grid_search"] == dict(C["keys"][i], ddg_step=int(got["j"][i]) * 8, ddg_delta=int(got["dmax"][i]))


def test_chunking_and_a_second_run_give_the_same_bits():
    from mapf_gpt_amd import ddg
    C = _policy_run()
    assert_same_bits(ddg.collect(C["run"], C["case"]["grids"], C["case"]["goal"], C["keys"], max_teacher_instances=3, **C["kw"]), C["out"])
    assert_same_bits(ddg.collect(C["run"], C["case"]["grids"], C["case"]["goal"], C["keys"], **C["kw"]), C["out"])


def test_a_lifelong_group_raises():
    import torch
    from mapf_gpt_amd import ddg
    from mapf_gpt_amd.model import build_model
    from mapf_gpt_amd.runner import BatchedRunner
    case = er.random_case(10, 10, 0.2, 2, 4, 8, seed=1)
    run = BatchedRunner(case["grids"], 2, 4, build_model("tiny", seed=0, max_rows=64, precision="f32"), max_episode_steps=8, precision="f32",
                        record=True)
    queue = torch.from_numpy(np.broadcast_to(case["goal"][:, :, None, :], (2, 4, 3, 2)).copy())
    run.reset(torch.from_numpy(case["pos"]), torch.from_numpy(case["goal"]), goal_queue=queue)
    run.run(8)
    pos, act, lengths = run.trajectory()                                  # recording itself works in a lifelong episode
    assert np.array_equal(pos[8].cpu().numpy(), run.env.sync_state()[0].cpu().numpy()) and lengths.tolist() == [8, 8]
    with pytest.raises(NotImplementedError, match="joint goal"):
        ddg.collect(run, case["grids"], case["goal"], [{}, {}])
    with pytest.raises(NotImplementedError, match="joint goal"):
        ddg.collect_from_trajectory(case["grids"], pos, lengths, case["goal"], [{}, {}], on_target="restart")


def test_the_cli_log_goes_through_split_by_map_and_the_dataset_tokenizer(tmp_path, capfd):
    import yaml
    from mapf_gpt_amd import dataset_build, ddg, maps
    from mapf_gpt_amd import dataset_tokenizer as dt
    from mapf_gpt_amd import evaluation as ev
    cfg = ev.load_yaml(os.path.join(ROOT, "eval_configs", "00-smoke", "00-smoke.yaml"))
    cfg["environment"].update(num_agents=8, max_episode_steps=32, seed={"grid_search": [0, 1]})
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    argv = ["--weights", "synthetic:tiny", "--config", str(tmp_path / "cfg.yaml"), "--out", str(tmp_path / "out"), "--every", "8",
            "--max-iters", "256", "--refine-rounds", "2", "--precision", "f32", "--seed", "1"]
    assert ddg.main(argv) == 0
    line = json.loads(capfd.readouterr().out.strip().splitlines()[-1])
    assert set(line) == {"episodes", "snapshots", "picked", "teacher_solved", "rows", "delta_mean", "delta_max", "seconds"}
    assert set(line["seconds"]) == {"rollout", "probe", "pick", "teacher"} and line["episodes"] == 4 and line["snapshots"] <= 4 * 5
    per_map = dataset_build.split_by_map(str(tmp_path / "out" / "DDG.json"), str(tmp_path / "temp"))
    res = [r for v in per_map.values() for r in v]
    assert len(res) == line["picked"] and all(r["algorithm"] == "DDG" for r in res)
    assert all(r["env_grid_search"]["ddg_step"] % 8 == 0 and "ddg_delta" in r["env_grid_search"] for r in res)
    assert line["teacher_solved"] == sum(r["metrics"]["CSR"] >= 1 for r in res)
    named = {k: "\n".join(v) for k, v in maps.named_maps().items() if k.startswith("validation-")}
    inputs, labels = dt.ObservationGenerator(named, res).generate_observations(0, len(res))
    want = sum(len(g) for r in res if r["metrics"]["CSR"] >= 1 for g in dt.gt_actions(r["metrics"]["made_actions"]))     # the tokenizer's own rule
    assert len(inputs) == len(labels) == want == line["rows"]
    assert want == sum((int(r["metrics"]["ep_length"]) + 1) * 8 for r in res if r["metrics"]["CSR"] >= 1)
