"""Batched episode tokenizer on the device: mgpt_dataset_episode_offsets / mgpt_dataset_tokenize_episodes through
dataset_tokenizer.tokenize_episodes against the reference's goldens and the pinned restatement, BatchedExpert.dataset_rows and
dataset_build.EpisodeStore against the per-episode route (records() -> generate_observations_device, split_by_map -> build_shards),
and the two CLIs' --shards."""
import glob
import json
import os

import numpy as np
import pytest

from mapf_gpt_amd import maps
from tests import episode_rows_ref as rr

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_tables = {}


def table(grid):
    from mapf_gpt_amd.dataset_tokenizer import MapTable
    key = (np.asarray(grid).shape, np.asarray(grid).tobytes())
    if key not in _tables:
        _tables[key] = MapTable(grid)
    return _tables[key]


def run(grid, init, actions, lengths, **kw):
    from mapf_gpt_amd.dataset_tokenizer import tokenize_episodes
    x, y, r = tokenize_episodes(table(grid), init, actions, np.asarray(lengths, np.int32), **kw)
    assert x.is_cuda and y.is_cuda and r.is_cuda and x.shape[0] == y.shape[0]
    return x.cpu().numpy(), y.cpu().numpy(), r.cpu().numpy()


def assert_equal(got, want):
    assert got[2].tolist() == want[2].tolist()
    assert got[0].shape == want[0].shape and np.array_equal(got[1], want[1])
    bad = np.nonzero((got[0] != want[0]).any(1))[0]
    assert len(bad) == 0, f"{len(bad)} rows differ, first {bad[:5]}"


@pytest.mark.parametrize("name", ["ds_maze", "ds_random", "ds_short", "ds_maskc2g"])
def test_reference_goldens_as_a_batch_of_three_with_the_middle_one_skipped(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    n, T = g["made_actions"].shape
    init = np.stack([g["init_positions"]] * 3).astype(np.int16)
    actions = np.stack([g["made_actions"]] * 3).astype(np.int8)
    x, y, row0 = run(g["grid"], init, actions, [T] * 3, keep=[1, 0, 1], mask_cost2go="mask_cost2go" in g)
    R = n * (T + 1)
    assert row0.tolist() == [0, R, R, 2 * R]
    assert np.array_equal(x.view(np.int8), np.concatenate([g["inputs"]] * 2))
    assert np.array_equal(y, np.concatenate([g["gt_actions"]] * 2))


@pytest.fixture(scope="module")
def ragged():
    """9 x 11 at 20 %, 7 agents, cap 6, lengths 6 (the cap), 1, 0, 3, 6, 2."""
    grid = maps.pad(maps.random_map(9, 11, 0.2, 33))
    lengths = [6, 1, 0, 3, 6, 2]
    init, actions = rr.random_walks(grid, 6, 7, 6, lengths, seed=5)
    return dict(grid=grid, init=init, actions=actions, lengths=lengths)


@pytest.mark.parametrize("keep", [None, [0, 1, 1, 0, 1, 0]], ids=["all", "some"])
def test_ragged_batch_against_the_restatement(ragged, keep):
    b = ragged
    got = run(b["grid"], b["init"], b["actions"], b["lengths"], keep=keep)
    assert got[0].shape[0] == 7 * sum(l + 1 for l, k in zip(b["lengths"], keep or [1] * 6) if k)
    assert_equal(got, rr.expected(b["grid"], b["init"], b["actions"], b["lengths"], keep))


@pytest.mark.parametrize("n_agents,h,w,lengths", [(5, 21, 21, [3, 2]), (16, 21, 21, [3, 2]), (17, 21, 21, [3, 2]), (70, 21, 21, [3, 2]),
                                                   (150, 30, 34, [3, 3])])
def test_agent_count_edges(n_agents, h, w, lengths):
    """16 agents per workgroup and the 64-lane candidate loop: one under, at and one over a chunk; more than a wave; 150 agents in
    crowded windows (more than 13 candidates)."""
    grid = maps.pad(maps.random_map(h, w, 0.12, 70 + n_agents))
    init, actions = rr.random_walks(grid, 2, n_agents, 3, lengths, seed=n_agents)
    assert_equal(run(grid, init, actions, lengths), rr.expected(grid, init, actions, lengths))


@pytest.mark.parametrize("mask", [False, True], ids=["cost2go", "mask_cost2go"])
@pytest.mark.parametrize("n_agents", rr.CROWDED["n_agents"])
def test_crowded_windows_against_the_restatement(n_agents, mask):
    """129 and 150 agents on 30 x 34 at 15 %: three 64-lane candidate passes, the last one partial, in the one row body every route
    shares.  No window holds more agents than the 128 candidates the kernels keep, so the restatement is the rows' definition here."""
    grid, init, actions, lengths, most = rr.crowded_case(n_agents)
    assert most <= 128
    assert_equal(run(grid, init, actions, lengths, mask_cost2go=mask), rr.expected(grid, init, actions, lengths, mask_cost2go=mask))


def _launches(name):
    from mapf_gpt_amd import _lib
    return _lib.prof_read().get(name, (0.0, 0))[1]


def test_selection_order_keep_on_top_and_empty_selections(ragged):
    from mapf_gpt_amd import _lib
    import torch
    b = ragged
    args = (b["grid"], b["init"], b["actions"], b["lengths"])
    keep = [0, 1, 1, 0, 1, 0]
    for ep in ([4, 1, 5], np.array([4, 1, 5]), torch.tensor([4, 1, 5], device="cuda")):
        assert_equal(run(*args, episodes=ep), rr.expected(*args, None, [4, 1, 5]))
        got = run(*args, keep=keep, episodes=ep)
        assert got[2].tolist() == [0, 49, 63, 63]                          # 4 kept (7 x 7 rows), 1 kept (7 x 2), 5 skipped
        assert_equal(got, rr.expected(*args, keep, [4, 1, 5]))
    with pytest.raises(IndexError):
        run(*args, episodes=[4, 6])
    with pytest.raises(IndexError):
        run(*args, episodes=torch.tensor([-1, 2], device="cuda"))
    _lib.prof_enable(True)
    try:
        _lib.prof_reset()
        x, y, row0 = run(*args, episodes=[])
        assert x.shape == (0, 256) and y.shape == (0,) and row0.tolist() == [0]
        x, y, row0 = run(*args, keep=[0] * 6)
        assert x.shape == (0, 256) and y.shape == (0,) and row0.tolist() == [0] * 7
        assert _launches("ds_episode_tokens") == 0 and _launches("ds_paths") == 0
        run(*args)
        assert _launches("ds_episode_tokens") == 1 and _launches("ds_paths") == 1
    finally:
        _lib.prof_enable(False)


def test_splitting_and_a_second_run_give_the_same_bits(ragged):
    b = ragged
    args = (b["grid"], b["init"], b["actions"], b["lengths"])
    keep = [1, 1, 0, 1, 1, 1]
    one = run(*args, keep=keep, episodes=[5, 0, 2, 4, 1])
    for again in (run(*args, keep=keep, episodes=[5, 0, 2, 4, 1]),
                  run(*args, keep=keep, episodes=[5, 0, 2, 4, 1], max_rows_per_call=50),      # 49 rows per episode at most: one per call
                  run(*args, keep=keep, episodes=[5, 0, 2, 4, 1], max_rows_per_call=100)):    # two per call
        assert all(np.array_equal(a, c) for a, c in zip(one, again))
    assert_equal(one, rr.expected(*args, keep, [5, 0, 2, 4, 1]))
    whole = run(*args)
    assert all(np.array_equal(a, c) for a, c in zip(whole, run(*args, max_rows_per_call=50)))


def test_bad_action_bytes_and_lengths_are_clamped(ragged):
    b = ragged
    actions, lengths = b["actions"].copy(), list(b["lengths"])
    # bad bytes go where the walk waited, so that the log as the device reads it is still a walk on free cells
    for e, bad in ((3, (9, -7)), (4, (9, -7, 127))):                       # 3 is skipped below, 4 is kept
        waits = np.argwhere(actions[e, :, :b["lengths"][e]] == 0)
        assert len(waits) >= len(bad)
        for (a, t), v in zip(waits, bad):
            actions[e, a, t] = v
    lengths[0] = lengths[3] = lengths[4] = 6 + 3                           # 0 and 4 kept, 3 skipped
    keep = [1, 1, 1, 0, 1, 1]
    got = run(b["grid"], b["init"], actions, lengths, keep=keep)
    assert got[2].tolist() == [0, 49, 63, 70, 70, 119, 140]
    assert_equal(got, rr.expected(b["grid"], b["init"], actions, lengths, keep))
    clean, cut = rr.clamped(actions, lengths, 6)
    assert np.array_equal(clean, b["actions"]) and (actions != clean).sum() == 5 and cut.tolist() == [6, 1, 0, 6, 6, 2]
    assert all(np.array_equal(a, c) for a, c in zip(got, run(b["grid"], b["init"], clean, cut, keep=keep)))


# ---- BatchedExpert.dataset_rows ------------------------------------------------------------------------------------------------------
def _per_episode_route(case, ex, ids, name, obst):
    from mapf_gpt_amd.dataset_tokenizer import ObservationGenerator
    keys = [{"map_name": case["names"][i % 2], "seed": i} for i in range(rr.ROWS_CASE["n_inst"])]
    recs = [r for i, r in enumerate(ex.records(keys, case["pos"])) if i in set(ids.tolist())]
    assert all(r["env_grid_search"]["map_name"] == name for r in recs)
    x, y = ObservationGenerator({name: rr.map_string(obst)}, recs).generate_observations_device(0, len(recs))
    return x.cpu().numpy(), y.cpu().numpy(), recs


@pytest.mark.parametrize("search", [None, "lacam"])
def test_expert_dataset_rows_equal_the_per_episode_route_map_by_map(search):
    import torch
    from mapf_gpt_amd.dataset_tokenizer import TableCache
    from mapf_gpt_amd.expert import BatchedExpert
    c, case = rr.ROWS_CASE, rr.rows_case()
    assert case["grids"].shape == (2, 20, 22)                               # 10 x 10 and 8 x 12 in one frame
    kw = dict(search="lacam", max_iters=256) if search else {}
    ex = BatchedExpert(case["grids"], c["n_inst"], c["n_agents"], c["cap"], seed=c["seed"], **kw)
    ex.reset(torch.from_numpy(case["pos"]), torch.from_numpy(case["goal"]))
    ex.run(c["cap"])
    csr = ex.metrics()[:, 0].cpu().numpy()
    if not search:
        assert csr.tolist() == c["csr"] and ex.log()[1].cpu().tolist() == c["lengths"]
        assert (csr >= 1).any() and (csr < 1).any()                         # a solved and an unsolved episode, as chosen on the CPU
    cache = TableCache()
    out = ex.dataset_rows(case["pos"], tables=cache)
    assert [ids.tolist() for ids, _, _ in out] == [[0, 2], [1, 3]] and cache.builds == 2
    total = 0
    for (ids, x, y), name, obst in zip(out, case["names"], case["obst"]):
        wx, wy, recs = _per_episode_route(case, ex, ids, name, obst)
        assert x.is_cuda and np.array_equal(x.cpu().numpy(), wx) and np.array_equal(y.cpu().numpy(), wy)
        assert len(wx) == sum(c["n_agents"] * (int(r["metrics"]["ep_length"]) + 1) for r in recs if r["metrics"]["CSR"] >= 1)
        total += len(wx)
    assert total > 0
    if not search:                                                           # instance 0 is unsolved: the first map's rows are instance 2's
        assert out[0][1].shape[0] == c["n_agents"] * (c["lengths"][2] + 1)
    # keep=None keeps the unsolved ones too; a tensor is used as given; the cache builds no table twice
    every = ex.dataset_rows(case["pos"], keep=None, tables=cache, offsets=True)
    lens = ex.log()[1].cpu().numpy()
    assert [r.cpu().tolist() for _, _, _, r in every] == [np.cumsum([0] + [c["n_agents"] * (int(lens[i]) + 1) for i in ids]).tolist()
                                                           for ids in ([0, 2], [1, 3])]
    only3 = ex.dataset_rows(case["pos"], keep=torch.tensor([False, False, False, True]), tables=cache)
    assert only3[0][1].shape[0] == 0 and only3[1][1].shape[0] == c["n_agents"] * (int(lens[3]) + 1) and cache.builds == 2


def test_a_lifelong_expert_raises_and_names_records():
    from mapf_gpt_amd.expert import BatchedExpert
    case = rr.rows_case()
    ex = BatchedExpert(case["grids"], 4, 6, 8, lifelong=True)
    with pytest.raises(NotImplementedError, match=r"records\(\)"):
        ex.dataset_rows(case["pos"])


# ---- shards ----------------------------------------------------------------------------------------------------------------------------
def _tiny_maps():
    """Two mazes and two random maps small enough for PIBT at a 16-step cap (tests/expert_ref.py on the CPU: 4 and 6 agents, seeds 0 and 1
    give solved and unsolved episodes on the mazes, solved ones on the random maps)."""
    return {"tiny-mazes-0": rr.map_string(maps.maze_map(5, 9, 3)), "tiny-mazes-1": rr.map_string(maps.maze_map(5, 9, 4)),
            "tiny-random-0": rr.map_string(maps.random_map(8, 9, 0.15, 3)), "tiny-random-1": rr.map_string(maps.random_map(9, 8, 0.15, 4))}


def _config():
    return {"environment": {"name": "Environment", "with_animation": False, "on_target": "nothing", "max_episode_steps": 16,
                            "observation_type": "MAPF", "collision_system": "soft", "seed": {"grid_search": [0, 1]},
                            "num_agents": {"grid_search": [4, 6]}, "map_name": {"grid_search": list(_tiny_maps())}},
            "algorithms": {"PIBT": {"name": "PIBT", "seed": 0, "device": "cuda"}}}


def _shard_bytes(prefix):
    files = sorted(glob.glob(prefix + "*_part_*.arrow"))
    return {os.path.basename(f)[len(os.path.basename(prefix)):]: open(f, "rb").read() for f in files}


def _counters(reports):
    return [{"files": r["files"], "rows": r["rows"], "shards": [s["rows"] for s in r["shards"]]} for r in reports]


@pytest.fixture(scope="module")
def expert_run(tmp_path_factory):
    from mapf_gpt_amd import dataset_build as db
    from mapf_gpt_amd import evaluation as ev
    d = tmp_path_factory.mktemp("episode_rows")
    reg = ev.MapRegistry()
    reg.register_maps(_tiny_maps())
    store = db.EpisodeStore()
    res = ev.evaluation(_config(), eval_dir=str(d / "out"), registry=reg, print_fn=lambda *_: None, log_actions=True,
                        on_expert_batch=store.append)
    per_map = db.split_by_map(str(d / "out" / "PIBT.json"), str(d / "temp"))
    files = [str(d / "temp" / f"{n}.json") for n in per_map]
    return dict(dir=d, store=store, res=res, files=files)


CUTS = [dict(desired_size=10 ** 6, files_per_chunk=3, num_chunks=1), dict(desired_size=150, files_per_chunk=2, num_chunks=2, maze_ratio=0.6)]


@pytest.mark.parametrize("cut", CUTS, ids=["everything", "two_chunks_small"])
def test_store_shards_are_the_log_routes_bytes(expert_run, cut):
    from mapf_gpt_amd import dataset_build as db
    r = expert_run
    solved = [x for x in r["res"] if x["metrics"]["CSR"] >= 1]
    assert 0 < len(solved) < len(r["res"]) == r["store"].episodes() == 16
    assert r["store"].solved_rows() == (len(solved), sum(len(x["metrics"]["made_actions"]) * (int(x["metrics"]["ep_length"]) + 1) for x in solved))
    tag = f"{cut['num_chunks']}_{cut['desired_size']}"
    os.makedirs(r["dir"] / ("log" + tag))
    os.makedirs(r["dir"] / ("dev" + tag))
    a = db.build_shards(_tiny_maps(), _tiny_maps(), r["files"], str(r["dir"] / ("log" + tag) / "chunk"), seed=3, **cut)
    b = db.build_shards_from_store(r["store"], str(r["dir"] / ("dev" + tag) / "chunk"), seed=3, **cut)
    assert _counters(a) == _counters(b) and sum(rep["rows"] for rep in a) > 0
    if cut["num_chunks"] == 2:                                               # below the total: the picks decide
        assert all(rep["rows"] <= 150 for rep in a) and any(f["picked"] < f["kept"] for rep in a for f in rep["files"])
    fa, fb = _shard_bytes(str(r["dir"] / ("log" + tag) / "chunk")), _shard_bytes(str(r["dir"] / ("dev" + tag) / "chunk"))
    assert len(fa) == cut["files_per_chunk"] * cut["num_chunks"] and fa == fb


def test_expert_cli_shards_reproduce_the_files(expert_run, tmp_path, capfd):
    import yaml
    from mapf_gpt_amd import dataset_build as db
    from mapf_gpt_amd import expert
    r = expert_run
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(_config(), f, sort_keys=False)         # the grid search runs its keys in the order written: keep the fixture's
    with open(tmp_path / "maps.yaml", "w") as f:
        yaml.safe_dump(_tiny_maps(), f)
    argv = ["--config", str(tmp_path / "cfg.yaml"), "--maps", str(tmp_path / "maps.yaml"), "--shards", str(tmp_path / "cli" / "chunk"),
            "--desired-size", "150", "--maze-ratio", "0.6", "--files-per-chunk", "2", "--num-chunks", "2", "--shard-seed", "3"]
    assert expert.main(argv) == 0
    line = json.loads(capfd.readouterr().out.strip().splitlines()[-1])
    assert set(line) == {"episodes", "solved", "rows", "seconds", "chunks"} and line["episodes"] == 16
    assert (line["solved"], line["rows"]) == r["store"].solved_rows() and not os.path.exists(tmp_path / "cli" / "PIBT.json")
    os.makedirs(tmp_path / "want")
    want = db.build_shards_from_store(r["store"], str(tmp_path / "want" / "chunk"), 150, 0.6, 2, 2, 3)
    assert _counters(line["chunks"]) == _counters(want)
    assert _shard_bytes(str(tmp_path / "cli" / "chunk")) == _shard_bytes(str(tmp_path / "want" / "chunk"))
    # with --out as well the JSON log is written too
    assert expert.main(argv + ["--out", str(tmp_path / "both")]) == 0
    capfd.readouterr()
    assert len(json.load(open(tmp_path / "both" / "PIBT.json"))) == 16


def test_ddg_rows_are_the_tokenizers_rows_of_its_records():
    from mapf_gpt_amd import ddg
    from mapf_gpt_amd.dataset_tokenizer import ObservationGenerator
    from tests import ddg_ref as dr
    h = dr.hand_trajectory()
    out = ddg.collect_from_trajectory(h["grids"], h["pos_traj"], h["lengths"], h["goal"], h["run_keys"], every=h["every"], rows=True)
    recs = out["records"]
    assert len(recs) == 1 and recs[0]["metrics"]["CSR"] == 1.0
    x, y = ObservationGenerator({"empty8": rr.map_string(h["grids"][5:-5, 5:-5])}, recs).generate_observations_device(0, 1)
    assert out["rows"].is_cuda and out["rows"].shape[0] == 3 * (int(recs[0]["metrics"]["ep_length"]) + 1)
    assert np.array_equal(out["rows"].cpu().numpy(), x.cpu().numpy()) and np.array_equal(out["labels"].cpu().numpy(), y.cpu().numpy())
    plain = ddg.collect_from_trajectory(h["grids"], h["pos_traj"], h["lengths"], h["goal"], h["run_keys"], every=h["every"])
    assert "rows" not in plain and plain["records"] == recs


def test_ddg_cli_shards_read_back_through_the_training_loader(tmp_path, capfd):
    import yaml
    from mapf_gpt_amd import ddg
    from mapf_gpt_amd import evaluation as ev
    from mapf_gpt_amd.scoring import read_arrow
    from mapf_gpt_amd.training import ArrowBatches
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = ev.load_yaml(os.path.join(root, "eval_configs", "00-smoke", "00-smoke.yaml"))
    cfg["environment"].update(num_agents=8, max_episode_steps=32, seed={"grid_search": [0, 1]})
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    argv = ["--weights", "synthetic:tiny", "--config", str(tmp_path / "cfg.yaml"), "--every", "8", "--max-iters", "256", "--refine-rounds", "2",
            "--precision", "f32", "--seed", "1", "--shards", str(tmp_path / "shards" / "chunk"), "--desired-size", "100000", "--files-per-chunk", "2"]
    assert ddg.main(argv) == 0
    line = json.loads(capfd.readouterr().out.strip().splitlines()[-1])
    assert "chunks" in line and "shards" in line["seconds"] and not os.path.exists(tmp_path / "shards" / "DDG.json")
    rep = line["chunks"][0]
    assert line["teacher_solved"] >= 1 and sum(f["samples"] for f in rep["files"]) == line["rows"] and 0 < rep["rows"] <= line["rows"]
    files = sorted(glob.glob(str(tmp_path / "shards" / "chunk_part_*.arrow")))
    assert len(files) == 2 and sum(len(read_arrow(f)[0]) for f in files) == rep["rows"]
    xb, tb = next(iter(ArrowBatches(str(tmp_path / "shards"), 16)))
    assert xb.shape == (16, 256) and ((tb[:, -1] >= 0) & (tb[:, -1] <= 4)).all()
