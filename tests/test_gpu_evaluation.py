"""Evaluation harness on the device: the smoke config end to end, result schema, determinism, metric sanity."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_smoke_config_end_to_end(tmp_path):
    from mapf_gpt_amd import evaluation as ev
    cfg = ev.load_yaml(os.path.join(ROOT, "eval_configs", "00-smoke", "00-smoke.yaml"))
    cfg["algorithms"]["MAPF-GPT-2M"]["path_to_weights"] = "synthetic:tiny"
    lines = []
    res = ev.evaluation(cfg, eval_dir=str(tmp_path), print_fn=lines.append)
    assert len(res) == 16
    assert os.path.exists(tmp_path / "MAPF-GPT-2M.json")
    for r in res:
        assert set(r) == {"metrics", "env_grid_search", "algorithm"}
        assert set(r["env_grid_search"]) == {"seed", "num_agents", "map_name"}
        m = r["metrics"]
        assert set(m) == {"CSR", "ISR", "SoC", "makespan", "ep_length", "avg_agents_density", "runtime"}
        assert 0.0 < m["avg_agents_density"] <= 1.0
        assert 0.0 <= m["ISR"] <= 1.0 and m["CSR"] in (0.0, 1.0) and 0 < m["ep_length"] <= 64
        assert m["makespan"] <= m["ep_length"] and m["SoC"] <= r["env_grid_search"]["num_agents"] * m["ep_length"]
    assert lines[0] == "== TabularView1" and lines[1].split()[:2] == ["num_agents", "algorithm"]
    res2 = ev.evaluation(cfg, print_fn=lambda *_: None)
    key = lambda r: tuple(sorted(r["env_grid_search"].items()))
    a = {key(r): [r["metrics"][k] for k in ev.METRIC_KEYS] for r in res}
    b = {key(r): [r["metrics"][k] for k in ev.METRIC_KEYS] for r in res2}
    assert a == b                                              # same seeds, same device sampler -> same episodes


def test_batch_composition_does_not_change_an_episode():
    """An instance's episode depends on its own (map, seed, agents) only: running it inside a bigger batch (other maps
    padded to a larger common frame) gives the same metrics as running it alone."""
    from mapf_gpt_amd import evaluation as ev
    base = {"environment": {"name": "Environment", "on_target": "nothing", "max_episode_steps": 32, "seed": 3, "num_agents": 8,
                            "map_name": {"grid_search": ["validation-random-seed-000"]}},
            "algorithms": {"A": {"name": "MAPF-GPT", "path_to_weights": "synthetic:tiny", "precision": "f16x3"}}}
    alone = ev.evaluation(base, print_fn=lambda *_: None)
    base["environment"]["map_name"]["grid_search"] = ["wfi_warehouse", "validation-random-seed-000"]
    both = ev.evaluation(base, print_fn=lambda *_: None)
    m0 = [alone[0]["metrics"][k] for k in ("CSR", "ISR", "SoC", "makespan", "ep_length")]
    m1 = [both[1]["metrics"][k] for k in ("CSR", "ISR", "SoC", "makespan", "ep_length")]
    assert both[1]["env_grid_search"]["map_name"] == "validation-random-seed-000"
    assert m0 == m1


def test_lifelong_config_reports_throughput():
    from mapf_gpt_amd import evaluation as ev
    cfg = {"environment": {"name": "Environment", "on_target": "restart", "max_episode_steps": 32, "num_agents": 8,
                           "seed": {"grid_search": [0, 1]}, "map_name": "validation-random-seed-000"},
           "algorithms": {"A": {"name": "MAPF-GPT", "path_to_weights": "synthetic:tiny", "precision": "f16x3"}},
           "results_views": {"T": {"type": "tabular", "drop_keys": ["seed"], "print_results": True}}}
    lines = []
    res = ev.evaluation(cfg, print_fn=lines.append)
    assert len(res) == 2
    for r in res:
        assert set(r["metrics"]) == {"avg_throughput", "ep_length", "runtime"}
        assert r["metrics"]["ep_length"] == 32 and r["metrics"]["avg_throughput"] >= 0.0
    assert "avg_throughput" in lines[1]


# ----------------------------------------------------------------------------------------------------------------------
# harness output vs an oracle replay of the same episodes (benchmark.py:20-50,
# eval_configs/01-random/01-random.yaml:1-10,145-186, experiment_setup/create_env.py:14-20,38-40)
# ----------------------------------------------------------------------------------------------------------------------
def _replay_metrics(grid, pos0, goal, actions, max_steps):
    """One episode replayed on the host from the device's sampled actions: the C oracle's env step (our spec)
    and an INDEPENDENT computation of the episode metrics from the whole trajectory (not the env kernel's incremental rule):
    the episode ends at the first step after which every agent stands on its goal, or at max_episode_steps; an agent's
    arrival time is the start of its final uninterrupted stay on the goal (0 if it never left it), ep_length otherwise."""
    from oracle import oracle as orc
    pos = pos0.astype(np.int32).copy()
    g = goal.astype(np.int32)
    traj = [pos.copy()]
    dens = [orc.agents_density(grid, pos)]
    T = 0
    for t in range(max_steps):
        pos, _ = orc.env_step(grid, pos, g, actions[t].astype(np.int32))
        traj.append(pos.copy())
        dens.append(orc.agents_density(grid, pos))
        T = t + 1
        if np.all(pos == g):
            break
    from tests.expert_checks import trajectory_metrics               # the one trajectory computation the expert's tests use too
    csr, isr, soc, makespan, ep_length = trajectory_metrics(np.stack(traj), g)
    assert ep_length == T
    return {"CSR": float(csr), "ISR": float(isr), "SoC": float(soc), "makespan": float(makespan), "ep_length": float(ep_length),
            "avg_agents_density": float(np.mean(dens))}


def _check_harness_against_replay(cfg, tmp_path):
    import json
    from mapf_gpt_amd import evaluation as ev
    log = []
    res = ev.evaluation(cfg, eval_dir=str(tmp_path), print_fn=lambda *_: None, trace=lambda kind, payload: log.append((kind, payload)))
    runs = ev.expand_grid_search(cfg["environment"])
    checked = 0
    for algo_name in cfg["algorithms"]:
        written = json.load(open(os.path.join(str(tmp_path), f"{algo_name}.json")))      # what the harness wrote
        by_point = {tuple(sorted(r["env_grid_search"].items())): r["metrics"] for r in written}
        assert len(by_point) == len(runs) == len(written)
        i = 0
        while i < len(log):
            kind, b = log[i]
            assert kind == "reset"
            steps = [p for k, p in log[i + 1:i + 1 + b["max_steps"]]]
            assert all(k == "step" for k, _ in log[i + 1:i + 1 + b["max_steps"]]) and len(steps) == b["max_steps"]
            i += 1 + b["max_steps"]
            if b["algorithm"] != algo_name:
                continue
            for k, ridx in enumerate(b["runs"]):
                want = _replay_metrics(b["grids"][k], b["pos"][k], b["goal"][k], [s[k] for s in steps], b["max_steps"])
                got = by_point[tuple(sorted(runs[ridx][1].items()))]
                for key in ("CSR", "ISR", "SoC", "makespan", "ep_length"):
                    assert got[key] == pytest.approx(want[key], rel=0, abs=1e-6), (runs[ridx][1], key, got[key], want[key])
                assert got["avg_agents_density"] == pytest.approx(want["avg_agents_density"], rel=2e-6), (runs[ridx][1], got, want)
                checked += 1
    assert checked == len(runs) * len(cfg["algorithms"])
    return res


def test_smoke_config_records_equal_an_oracle_replay(tmp_path):
    """eval_configs/00-smoke through evaluation(): every record of the JSON the harness writes (CSR, ISR, SoC, makespan,
    ep_length, avg_agents_density) equals the metrics of a host replay of that episode from the device's sampled actions."""
    from mapf_gpt_amd import evaluation as ev
    cfg = ev.load_yaml(os.path.join(ROOT, "eval_configs", "00-smoke", "00-smoke.yaml"))
    _check_harness_against_replay(cfg, tmp_path)


def test_reference_01_random_slice_equals_an_oracle_replay(tmp_path):
    """A 2-map x 2-agent-count slice of the reference's eval_configs/01-random/01-random.yaml (same environment block,
    lines 1-10; two of its maps ship in mapf_gpt_amd/data/named_maps.json) with both of its algorithm entries (2M and 6M
    shapes on synthetic weights): the second batch group and the 6M forward go through the same check; a greedy-looking
    policy on random weights rarely finishes, so CSR / SoC / makespan are exercised by a third, easy, configuration too."""
    cfg = {"environment": {"name": "Environment", "with_animation": False, "on_target": "nothing", "max_episode_steps": 128,
                           "observation_type": "MAPF", "collision_system": "soft", "seed": 0,
                           "num_agents": {"grid_search": [8, 16]},
                           "map_name": {"grid_search": ["validation-random-seed-000", "validation-random-seed-001"]}},
           "algorithms": {"MAPF-GPT-2M": {"name": "MAPF-GPT", "parallel_backend": "balanced_dask", "num_process": 4,
                                          "path_to_weights": "synthetic:2M"},
                          "MAPF-GPT-6M": {"name": "MAPF-GPT", "parallel_backend": "balanced_dask", "num_process": 4,
                                          "path_to_weights": "synthetic:6M"}},
           "results_views": {"TabularView1": {"type": "tabular", "drop_keys": ["seed", "map_name"], "print_results": True}}}
    _check_harness_against_replay(cfg, tmp_path)


def test_finishing_episodes_equal_an_oracle_replay(tmp_path):
    """Episodes that DO terminate (1 and 2 agents on an open map reach their goals by random walk within 256 steps often
    enough): CSR = 1, early ep_length, SoC / makespan from arrival times -- the branches a never-finishing policy skips."""
    cfg = {"environment": {"name": "Environment", "on_target": "nothing", "max_episode_steps": 256,
                           "seed": {"grid_search": list(range(12))}, "num_agents": {"grid_search": [1, 2]},
                           "map_name": "puzzle-00"},
           "algorithms": {"A": {"name": "MAPF-GPT", "path_to_weights": "synthetic:tiny", "precision": "f16x3"}}}
    res = _check_harness_against_replay(cfg, tmp_path)
    assert any(r["metrics"]["CSR"] == 1.0 for r in res), "no episode finished: the CSR = 1 branch went unchecked"


def test_two_ranks_write_the_single_rank_records(tmp_path):
    """benchmark.py under torch.distributed.run with 2 ranks (gloo, both on the one GPU): the instances of every batch are
    sharded over the ranks, the metric records gathered once -- and the JSON rank 0 writes equals the single-process one
    record for record (the device sampler is keyed by the global row, runtime excluded).  VERDICT r02 item 7c."""
    import json
    import shutil
    import subprocess
    import sys
    outs = {}
    for world in (1, 2):
        root = tmp_path / f"w{world}"
        shutil.copytree(os.path.join(ROOT, "eval_configs", "00-smoke"), root / "00-smoke")
        env = dict(os.environ, MGPT_BENCH_BACKEND="gloo", MGPT_BENCH_SHARE_GPU="1", MASTER_ADDR="127.0.0.1")
        cmd = [sys.executable, os.path.join(ROOT, "benchmark.py"), "--eval-root", str(root), "--folders", "00-smoke"]
        if world > 1:
            cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
                   "--master-port", "29547"] + cmd[1:]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        recs = json.load(open(root / "00-smoke" / "MAPF-GPT-2M.json"))
        outs[world] = {tuple(sorted(x["env_grid_search"].items())): {k: v for k, v in x["metrics"].items() if k != "runtime"} for x in recs}
    assert len(outs[1]) == 16 and outs[1] == outs[2]
