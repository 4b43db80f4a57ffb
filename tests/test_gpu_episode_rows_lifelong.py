"""Lifelong batched episode tokenizer on the device: mgpt_dataset_tokenize_episodes_lifelong through
dataset_tokenizer.tokenize_episodes(targets=, n_targets=) against the reference's lifelong goldens, the pinned restatement and the
per-episode route (MapTable.tokenize with goals), BatchedExpert.lifelong_rows / lifelong_targets against records() ->
generate_observations_device, EpisodeStore(lifelong=True) and `expert --lifelong-shards` against split_by_map -> build_shards."""
import glob
import json
import os

import numpy as np
import pytest

from mapf_gpt_amd import maps
from tests import episode_rows_lifelong_ref as lr
from tests import episode_rows_ref as rr
from tests import expert_lifelong_ref as xr

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_tables = {}


def table(grid):
    from mapf_gpt_amd.dataset_tokenizer import MapTable
    key = (np.asarray(grid).shape, np.asarray(grid).tobytes())
    if key not in _tables:
        _tables[key] = MapTable(grid)
    return _tables[key]


def run(grid, init, actions, lengths, targets, n_targets=None, **kw):
    from mapf_gpt_amd.dataset_tokenizer import tokenize_episodes
    x, y, r = tokenize_episodes(table(grid), init, actions, np.asarray(lengths, np.int32), targets=targets, n_targets=n_targets, **kw)
    assert x.is_cuda and y.is_cuda and r.is_cuda and x.shape[0] == y.shape[0]
    return x.cpu().numpy(), y.cpu().numpy(), r.cpu().numpy()


def assert_equal(got, want):
    assert got[2].tolist() == want[2].tolist()
    assert got[0].shape == want[0].shape and np.array_equal(got[1], want[1])
    bad = np.nonzero((got[0] != want[0]).any(1))[0]
    assert len(bad) == 0, f"{len(bad)} rows differ, first {bad[:5]}"


def per_episode_route(grid, init_e, actions_e, length, targets_e, n_targets_e=None, mask_cost2go=False):
    """MapTable.tokenize (the _ex call) on one episode's paths and per-step goals, labels from the numpy rule."""
    from mapf_gpt_amd import dataset_tokenizer as dt
    paths = lr.paths_of(init_e, actions_e, length)
    goals = dt.episode_goals(init_e, actions_e, length, targets_e, n_targets_e)
    x = table(grid).tokenize(paths, goals, mask_cost2go).reshape(-1, 256).cpu().numpy()
    return x, dt.episode_labels(actions_e, length).reshape(-1)


@pytest.mark.parametrize("name", ["ds_lifelong", "ds_lifelong_maze"])
def test_reference_lifelong_goldens_as_a_batch_of_three_with_the_middle_one_skipped(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    n, T = g["made_actions"].shape
    init = np.stack([g["init_positions"]] * 3).astype(np.int16)
    actions = np.stack([g["made_actions"]] * 3).astype(np.int8)
    targets = np.stack([g["lifelong_targets"]] * 3).astype(np.int16)          # plain lists of 24: L = 24, no wrap, n_targets = None
    x, y, row0 = run(g["grid"], init, actions, [T] * 3, targets, keep=[1, 0, 1])
    R = n * (T + 1)
    assert row0.tolist() == [0, R, R, 2 * R]
    assert np.array_equal(x.view(np.int8), np.concatenate([g["inputs"]] * 2))
    assert np.array_equal(y, np.concatenate([g["gt_actions"]] * 2))
    wx, wy = per_episode_route(g["grid"], g["init_positions"], g["made_actions"], T, g["lifelong_targets"])
    assert np.array_equal(x[:R], wx) and np.array_equal(y[:R], wy)


@pytest.mark.parametrize("keep", [None, [0, 1, 1, 0, 1, 0]], ids=["all", "some"])
@pytest.mark.parametrize("mask", [False, True], ids=["cost2go", "mask_cost2go"])
def test_base_case_against_the_restatement(keep, mask):
    b = lr.base_case()
    args = (b["grid"], b["init"], b["actions"], b["lengths"], b["targets"])
    got = run(*args, keep=keep, mask_cost2go=mask)
    assert got[0].shape[0] == 7 * sum(l + 1 for l, k in zip(b["lengths"], keep or [1] * 6) if k)
    assert_equal(got, lr.expected(*args, keep=keep, mask_cost2go=mask))
    if keep is None and not mask:                                            # the goals matter: episode 0 differs from the static-goal rows in every row
        static = rr.episode_rows(b["grid"], b["init"][0], b["actions"][0], 6)[0]
        assert (got[0][:49] != static).any(1).all()


def test_selection_order_splitting_and_a_second_run():
    import torch
    b = lr.base_case()
    args = (b["grid"], b["init"], b["actions"], b["lengths"], b["targets"])
    want = lr.expected(*args, episodes=[4, 1, 5])
    for ep in ([4, 1, 5], np.array([4, 1, 5]), torch.tensor([4, 1, 5], device="cuda")):
        assert_equal(run(*args, episodes=ep), want)
    keep = [1, 1, 0, 1, 1, 1]
    one = run(*args, keep=keep, episodes=[5, 0, 2, 4, 1])
    assert_equal(one, lr.expected(*args, keep=keep, episodes=[5, 0, 2, 4, 1]))
    for again in (run(*args, keep=keep, episodes=[5, 0, 2, 4, 1]),
                  run(*args, keep=keep, episodes=[5, 0, 2, 4, 1], max_rows_per_call=50),       # 49 rows per episode at most: one per call
                  run(*args, keep=keep, episodes=[5, 0, 2, 4, 1], max_rows_per_call=100)):     # two per call
        assert all(np.array_equal(a, c) for a, c in zip(one, again))
    whole = run(*args)
    assert all(np.array_equal(a, c) for a, c in zip(whole, run(*args, max_rows_per_call=50)))
    x, y, row0 = run(*args, episodes=[])
    assert x.shape == (0, 256) and y.shape == (0,) and row0.tolist() == [0]


@pytest.mark.parametrize("n_agents", [5, 16, 17, 70])
def test_agent_count_edges(n_agents):
    """16 agents per workgroup and the 64-lane candidate loop: one under, at and one over a chunk; more than a wave."""
    grid = maps.pad(maps.random_map(21, 21, 0.12, 70 + n_agents))
    lengths = [4, 2]
    init, actions = rr.random_walks(grid, 2, n_agents, 4, lengths, seed=n_agents)
    targets = lr.random_targets(grid, init, actions, lengths, seed=100 + n_agents)
    assert lr.goal_stats(grid, init, actions, lengths, targets)[0] >= n_agents // 5
    assert_equal(run(grid, init, actions, lengths, targets), lr.expected(grid, init, actions, lengths, targets))


@pytest.mark.parametrize("mask", [False, True], ids=["cost2go", "mask_cost2go"])
@pytest.mark.parametrize("n_agents", rr.CROWDED["n_agents"])
def test_crowded_windows_against_the_restatement(n_agents, mask):
    """The crowded case of tests/test_gpu_episode_rows.py with target lists: three 64-lane candidate passes, the last one partial, through
    the lifelong instantiation of the shared row body; no window holds more agents than the 128 candidates the kernels keep."""
    grid, init, actions, lengths, most = rr.crowded_case(n_agents)
    assert most <= 128
    targets = lr.random_targets(grid, init, actions, lengths, seed=100 + n_agents, within=12)     # 12 + cap 3 + radius 5 = 20
    assert lr.goal_stats(grid, init, actions, lengths, targets)[0] >= n_agents // 5
    assert_equal(run(grid, init, actions, lengths, targets, mask_cost2go=mask),
                 lr.expected(grid, init, actions, lengths, targets, mask_cost2go=mask))


def _oscillation():
    """Open 8 x 8, two agents: agent 0 walks x0 x1 x0 x1 x0 x1 with target(0) = x1 and the queue [x0, x1] (L = 3): it stands on the target
    it pursues at every t >= 1, so its list advances every step and wraps at t = 3.  Agent 1 stands next to it with a far goal."""
    grid = maps.pad(np.zeros((8, 8), np.uint8))
    x0, x1, far = (8, 8), (8, 9), (11, 12)
    init = np.array([[x0, (9, 8)]], np.int16)
    actions = np.array([[[4, 3, 4, 3, 4], [0, 0, 2, 0, 1]]], np.int8)
    targets = np.array([[[x1, x0, x1], [far, far, far]]], np.int16)
    return grid, init, actions, [5], targets


def test_the_list_wraps_as_the_expanded_list_does():
    grid, init, actions, lengths, targets = _oscillation()
    n_targets = np.array([[5 + 2, 1]], np.int32)
    got = run(grid, init, actions, lengths, targets, n_targets)
    assert lr.expand(targets[0, 0], 7) == [[8, 9], [8, 8], [8, 9], [8, 8], [8, 9], [8, 8], [8, 9]]
    assert_equal(got, lr.expected(grid, init, actions, lengths, targets, n_targets))
    wx, wy = per_episode_route(grid, init[0], actions[0], 5, targets[0], n_targets[0])
    assert np.array_equal(got[0], wx) and np.array_equal(got[1], wy)


def test_an_exhausted_list_raises_index_error_on_both_routes():
    """The defined error path: the walk flags the status word and goes on with the last valid index, every access in bounds."""
    from mapf_gpt_amd import dataset_tokenizer as dt
    grid, init, actions, lengths, targets = _oscillation()
    n_targets = np.array([[3, 1]], np.int32)
    with pytest.raises(IndexError):
        dt.goal_positions(lr.paths_of(init[0], actions[0], 5), [lr.expand(targets[0, 0], 3), lr.expand(targets[0, 1], 1)])
    with pytest.raises(IndexError):
        run(grid, init, actions, lengths, targets, n_targets)
    x, y, row0 = run(grid, init, actions, lengths, targets, n_targets, keep=[0])       # a skipped episode's lists are not walked
    assert x.shape == (0, 256) and row0.tolist() == [0, 0]
    assert run(grid, init, actions, [2], targets, n_targets)[0].shape == (6, 256)      # three targets last for two steps


def test_targets_outside_the_frame_and_bad_counts_in_a_skipped_episode():
    from mapf_gpt_amd import dataset_tokenizer as dt
    b = lr.base_case()
    targets = b["targets"].copy()
    L = targets.shape[2]
    n_targets = np.full((6, 7), L, np.int32)
    kept = (0, 1, 2, 4, 5)
    goals = {e: dt.episode_goals(b["init"][e], b["actions"][e], b["lengths"][e], targets[e]) for e in kept}
    first = [(e, a) for e in kept for a in range(7) if (goals[e][a, 0] != targets[e, a, 0]).any()]     # agents that advance at t = 0
    assert len(first) >= 3
    outside = [(30000, 2), (-3, 127), (127, -3)]
    for (e, a), cell in zip(first, outside):                                 # their second target: pursued from t = 0 on, never reached
        targets[e, a, 1] = cell
    rest = [(e, a) for e in kept for a in range(7) if (e, a) not in first][:3]
    for (e, a), cell in zip(rest, outside):                                  # the first target itself
        targets[e, a, 0] = cell
    targets[4, :, L - 1] = (-32768, 32767)
    n_targets[3] = 0                                                         # episode 3 is skipped: its counts are never read
    targets[3] = 30000
    keep = [1, 1, 1, 0, 1, 1]
    got = run(b["grid"], b["init"], b["actions"], b["lengths"], targets, n_targets, keep=keep)
    xs, ys = [], []
    for e in kept:
        x, y = per_episode_route(b["grid"], b["init"][e], b["actions"][e], b["lengths"][e], targets[e], n_targets[e])
        xs.append(x)
        ys.append(y)
    assert got[2].tolist() == [0, 49, 63, 70, 70, 119, 140]
    assert np.array_equal(got[0], np.concatenate(xs)) and np.array_equal(got[1], np.concatenate(ys))
    for (e, a), cell in list(zip(first, outside)) + list(zip(rest, outside)):          # pursued at every timestep of the episode
        assert (dt.episode_goals(b["init"][e], b["actions"][e], b["lengths"][e], targets[e], n_targets[e])[a] == cell).all()


def _launches(name):
    from mapf_gpt_amd import _lib
    return _lib.prof_read().get(name, (0.0, 0))[1]


def test_timing_hooks_tell_the_two_calls_apart():
    from mapf_gpt_amd import _lib
    from mapf_gpt_amd.dataset_tokenizer import tokenize_episodes
    b = lr.base_case()
    _lib.prof_enable(True)
    try:
        _lib.prof_reset()
        tokenize_episodes(table(b["grid"]), b["init"], b["actions"], np.asarray(b["lengths"], np.int32))
        assert _launches("ds_paths") == 1 and _launches("ds_episode_tokens") == 1
        assert _launches("ds_paths_lifelong") == 0 and _launches("ds_episode_tokens_lifelong") == 0
        _lib.prof_reset()
        run(b["grid"], b["init"], b["actions"], b["lengths"], b["targets"])
        assert _launches("ds_paths") == 0 and _launches("ds_episode_tokens") == 0
        assert _launches("ds_paths_lifelong") == 1 and _launches("ds_episode_tokens_lifelong") == 1
    finally:
        _lib.prof_enable(False)


# ---- BatchedExpert.lifelong_rows ---------------------------------------------------------------------------------------------------
def _expert_cases():
    c = xr.gpu_cases()
    return {"one_agent": c["one_agent"], "shared5": c["shared5"], "two_grids": xr.random_case(12, 12, 0.2, 4, 6, 24, seed=21, n_grids=2)}


@pytest.mark.parametrize("name", ["one_agent", "shared5", "two_grids"])
def test_expert_lifelong_rows_equal_the_per_episode_route(name):
    import torch
    from mapf_gpt_amd.dataset_tokenizer import ObservationGenerator, TableCache
    from mapf_gpt_amd.expert import BatchedExpert
    case = _expert_cases()[name]
    n_inst, n_agents, n_grids = case["n_inst"], case["n_agents"], len(case["grids"])
    ex = BatchedExpert(case["grids"], n_inst, n_agents, case["steps"], seed=case["seed"], inst_offset=case["inst_offset"], swap=case["swap"],
                       lifelong=True)
    with pytest.raises(RuntimeError, match=r"reset\(\)"):
        ex.lifelong_rows(case["pos"])
    with pytest.raises(RuntimeError, match=r"reset\(\)"):
        ex.lifelong_targets()
    ex.reset(torch.from_numpy(case["pos"]), torch.from_numpy(case["goal"]), torch.from_numpy(case["queue"]))
    ex.run(case["steps"])
    # lifelong_targets() is targets(), padded and expanded
    targets, n_targets = ex.lifelong_targets()
    Q = case["queue"].shape[2]
    assert targets.is_cuda and targets.dtype == torch.int16 and tuple(targets.shape) == (n_inst, n_agents, 1 + Q, 2)
    assert n_targets.is_cuda and n_targets.dtype == torch.int32 and tuple(n_targets.shape) == (n_inst, n_agents)
    tg, nt, host = targets.cpu().numpy(), n_targets.cpu().numpy(), ex.targets()
    assert [[lr.expand(tg[i, a], nt[i, a]) for a in range(n_agents)] for i in range(n_inst)] == host
    if name == "one_agent":
        assert nt.max() - 1 > Q                                              # more arrivals than queue entries: the list wraps
    names = [f"grid-{k}" for k in range(n_grids)]
    keys = [{"map_name": names[i % n_grids], "seed": i} for i in range(n_inst)]
    recs = ex.records(keys, case["pos"])
    named = {names[k]: rr.map_string(case["grids"][k][5:-5, 5:-5]) for k in range(n_grids)}
    cache = TableCache()
    out = ex.lifelong_rows(case["pos"], tables=cache, offsets=True)
    assert [ids.tolist() for ids, _, _, _ in out] == [list(range(k, n_inst, n_grids)) for k in range(n_grids)] and cache.builds == n_grids
    for k, (ids, x, y, row0) in enumerate(out):
        mine = [recs[i] for i in ids]
        wx, wy = ObservationGenerator(named, mine).generate_observations_device(0, len(mine))
        assert x.is_cuda and torch.equal(x, wx) and torch.equal(y, wy)
        assert row0.cpu().tolist() == [j * n_agents * (case["steps"] + 1) for j in range(len(ids) + 1)]      # every episode present, full length
    plain = ex.lifelong_rows(case["pos"], tables=cache)
    assert len(plain[0]) == 3 and torch.equal(plain[0][1], out[0][1]) and cache.builds == n_grids
    with pytest.raises(NotImplementedError, match=r"records\(\)"):           # dataset_rows keeps refusing a lifelong expert
        ex.dataset_rows(case["pos"])


def test_a_one_shot_expert_has_no_lifelong_rows():
    from mapf_gpt_amd.expert import BatchedExpert
    case = rr.rows_case()
    ex = BatchedExpert(case["grids"], 4, 6, 8)
    with pytest.raises(RuntimeError, match="lifelong=True"):
        ex.lifelong_rows(case["pos"])
    with pytest.raises(RuntimeError, match="lifelong=True"):
        ex.lifelong_targets()


# ---- shards ----------------------------------------------------------------------------------------------------------------------------
def _tiny_maps():
    return {"tiny-mazes-0": rr.map_string(maps.maze_map(5, 9, 3)), "tiny-mazes-1": rr.map_string(maps.maze_map(5, 9, 4)),
            "tiny-random-0": rr.map_string(maps.random_map(8, 9, 0.15, 3)), "tiny-random-1": rr.map_string(maps.random_map(9, 8, 0.15, 4))}


def _config():
    return {"environment": {"name": "Environment", "with_animation": False, "on_target": "restart", "max_episode_steps": 16,
                            "observation_type": "MAPF", "collision_system": "soft", "seed": {"grid_search": [0, 1]},
                            "num_agents": {"grid_search": [4, 6]}, "map_name": {"grid_search": list(_tiny_maps())}},
            "algorithms": {"PIBT": {"name": "PIBT", "seed": 0, "device": "cuda", "lifelong": True}}}


def _shard_bytes(prefix):
    files = sorted(glob.glob(prefix + "*_part_*.arrow"))
    return {os.path.basename(f)[len(os.path.basename(prefix)):]: open(f, "rb").read() for f in files}


def _counters(reports):
    return [{"files": r["files"], "rows": r["rows"], "shards": [s["rows"] for s in r["shards"]]} for r in reports]


@pytest.fixture(scope="module")
def expert_run(tmp_path_factory):
    from mapf_gpt_amd import dataset_build as db
    from mapf_gpt_amd import evaluation as ev
    d = tmp_path_factory.mktemp("episode_rows_lifelong")
    reg = ev.MapRegistry()
    reg.register_maps(_tiny_maps())
    store = db.EpisodeStore(lifelong=True)
    res = ev.evaluation(_config(), eval_dir=str(d / "out"), registry=reg, print_fn=lambda *_: None, log_actions=True,
                        on_expert_batch=store.append)
    per_map = db.split_by_map(str(d / "out" / "PIBT.json"), str(d / "temp"))
    files = [str(d / "temp" / f"{n}.json") for n in per_map]
    return dict(dir=d, store=store, res=res, files=files)


CUTS = [dict(desired_size=10 ** 6, files_per_chunk=3, num_chunks=1), dict(desired_size=150, files_per_chunk=2, num_chunks=2, maze_ratio=0.6)]


@pytest.mark.parametrize("cut", CUTS, ids=["everything", "two_chunks_small"])
def test_lifelong_store_shards_are_the_log_routes_bytes(expert_run, cut):
    from mapf_gpt_amd import dataset_build as db
    r = expert_run
    assert len(r["res"]) == r["store"].episodes() == 16 and all("CSR" not in x["metrics"] for x in r["res"])
    assert sum(len(tg) - 1 for x in r["res"] for tg in x["metrics"]["global_lifelong_targets_xy"]) > 0
    assert r["store"].solved_rows() == (16, sum(len(x["metrics"]["made_actions"]) * 17 for x in r["res"]))     # every episode, full length
    tag = f"{cut['num_chunks']}_{cut['desired_size']}"
    os.makedirs(r["dir"] / ("log" + tag))
    os.makedirs(r["dir"] / ("dev" + tag))
    a = db.build_shards(_tiny_maps(), _tiny_maps(), r["files"], str(r["dir"] / ("log" + tag) / "chunk"), seed=3, **cut)
    b = db.build_shards_from_store(r["store"], str(r["dir"] / ("dev" + tag) / "chunk"), seed=3, **cut)
    assert _counters(a) == _counters(b) and sum(rep["rows"] for rep in a) > 0
    if cut["num_chunks"] == 2:
        assert all(rep["rows"] <= 150 for rep in a) and any(f["picked"] < f["kept"] for rep in a for f in rep["files"])
    fa, fb = _shard_bytes(str(r["dir"] / ("log" + tag) / "chunk")), _shard_bytes(str(r["dir"] / ("dev" + tag) / "chunk"))
    assert len(fa) == cut["files_per_chunk"] * cut["num_chunks"] and fa == fb


def test_expert_cli_lifelong_shards_reproduce_the_files(expert_run, tmp_path, capfd):
    import yaml
    from mapf_gpt_amd import dataset_build as db
    from mapf_gpt_amd import expert
    r = expert_run
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(_config(), f, sort_keys=False)         # the grid search runs its keys in the order written: keep the fixture's
    with open(tmp_path / "maps.yaml", "w") as f:
        yaml.safe_dump(_tiny_maps(), f)
    argv = ["--config", str(tmp_path / "cfg.yaml"), "--maps", str(tmp_path / "maps.yaml"), "--lifelong-shards", str(tmp_path / "cli" / "chunk"),
            "--desired-size", "150", "--maze-ratio", "0.6", "--files-per-chunk", "2", "--num-chunks", "2", "--shard-seed", "3"]
    assert expert.main(argv) == 0
    line = json.loads(capfd.readouterr().out.strip().splitlines()[-1])
    assert set(line) == {"episodes", "rows", "seconds", "lifelong", "arrivals", "throughput", "chunks"} and line["episodes"] == 16
    assert line["rows"] == r["store"].solved_rows()[1] and not os.path.exists(tmp_path / "cli" / "PIBT.json")
    assert line["arrivals"] == sum(len(tg) - 1 for x in r["res"] for tg in x["metrics"]["global_lifelong_targets_xy"])
    os.makedirs(tmp_path / "want")
    want = db.build_shards_from_store(r["store"], str(tmp_path / "want" / "chunk"), 150, 0.6, 2, 2, 3)
    assert _counters(line["chunks"]) == _counters(want)
    assert _shard_bytes(str(tmp_path / "cli" / "chunk")) == _shard_bytes(str(tmp_path / "want" / "chunk"))
    # with --out as well the JSON log is written too
    assert expert.main(argv + ["--out", str(tmp_path / "both")]) == 0
    capfd.readouterr()
    assert len(json.load(open(tmp_path / "both" / "PIBT.json"))) == 16
