"""Retire mode, the parts that need no device: benchmark.py --retire-done and evaluation(retire_done=...) reach BatchedRunner, the
defaults stay off, and a runner that replays a hipGraph refuses the mode before it touches the device."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CFG = {"environment": {"name": "Environment", "on_target": "nothing", "max_episode_steps": 16, "num_agents": 2,
                       "seed": {"grid_search": [0, 1, 2]}, "map_name": "puzzle-00"},
       "algorithms": {"A": {"name": "MAPF-GPT", "path_to_weights": "synthetic:tiny"}}}


class _StubRunner:
    made = []

    def __init__(self, grids, n_inst, n_agents, net, **kw):
        self.n_inst, self.kw, self.ran = n_inst, kw, None
        _StubRunner.made.append(self)

    def reset(self, pos, goal, goal_queue=None):
        pass

    def run(self, steps):
        self.ran = steps

    def step(self):
        pass

    def metrics(self):
        return torch.zeros((self.n_inst, 6), dtype=torch.float32)


@pytest.fixture
def stubbed(monkeypatch):
    from mapf_gpt_amd import evaluation as ev, runner
    _StubRunner.made = []
    cfg = types.SimpleNamespace(seed=0, precision="f32", device="cpu", batch_size=1)
    monkeypatch.setattr(ev, "_build_algorithm", lambda algo_cfg, max_rows: (types.SimpleNamespace(net=None), cfg))
    monkeypatch.setattr(runner, "BatchedRunner", _StubRunner)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    return ev


@pytest.mark.parametrize("kw,want", [({}, False), ({"retire_done": False}, False), ({"retire_done": True}, True)])
def test_evaluation_hands_retire_done_to_the_runner(stubbed, kw, want):
    res = stubbed.evaluation(CFG, print_fn=lambda *_: None, **kw)
    assert len(res) == 3 and len(_StubRunner.made) == 1
    run = _StubRunner.made[0]
    assert run.kw["retire_done"] is want and run.ran == 16
    assert "use_graph" not in run.kw or not run.kw["use_graph"]


@pytest.mark.parametrize("flag,want", [([], False), (["--retire-done"], True)])
def test_benchmark_flag_reaches_evaluation(monkeypatch, tmp_path, flag, want):
    import importlib.util
    from mapf_gpt_amd import evaluation as ev, inference
    folder = tmp_path / "f0"
    folder.mkdir()
    import yaml
    (folder / "f0.yaml").write_text(yaml.safe_dump(CFG))
    seen = []
    monkeypatch.setattr(ev, "evaluation", lambda cfg, **kw: seen.append(kw) or [])
    monkeypatch.setattr(inference.MAPFGPTInference, "build", staticmethod(lambda *a, **k: None))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["benchmark.py", "--eval-root", str(tmp_path), "--folders", "f0"] + flag)
    spec = importlib.util.spec_from_file_location("_benchmark_under_test", os.path.join(ROOT, "benchmark.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main()
    assert len(seen) == 1 and seen[0]["retire_done"] is want


def test_graph_replay_with_retire_is_a_value_error():
    """Raised from the arguments alone, before the env / tokenizer contexts (which need a device) are built."""
    from mapf_gpt_amd.runner import BatchedRunner
    with pytest.raises(ValueError, match="use_graph"):
        BatchedRunner(np.zeros((12, 12), np.uint8), 1, 1, None, use_graph=True, retire_done=True)
    with pytest.raises(ValueError, match="poll_every"):
        BatchedRunner(np.zeros((12, 12), np.uint8), 1, 1, None, retire_done=True, poll_every=0)
