"""Host side of the lifelong batched episode tokenizer: the per-step goal rule as numpy states it against the two
restatements of the reference's get_goal_positions, the cyclic list addressing, the conditions on the base case's data, the lifelong
store's grouping and the CLI refusals.  No device."""
import json
import os

import numpy as np
import pytest

from mapf_gpt_amd import dataset_build as db
from mapf_gpt_amd import dataset_tokenizer as dt
from oracle import dataset_oracle as dso
from tests import episode_rows_lifelong_ref as lr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def both_restatements(paths, lists):
    a = dt.goal_positions(paths, lists)
    b = np.asarray(dso.goal_positions([[tuple(c) for c in p] for p in np.asarray(paths).tolist()], lists), np.int32)
    assert np.array_equal(a, b)
    return a


def test_episode_goals_on_the_base_case():
    b = lr.base_case()
    for e, ln in enumerate(b["lengths"]):
        paths = lr.paths_of(b["init"][e], b["actions"][e], ln)
        want = both_restatements(paths, [lr.expand(tg, len(tg)) for tg in b["targets"][e]])
        got = dt.episode_goals(b["init"][e], b["actions"][e], ln, b["targets"][e])
        assert got.shape == (7, ln + 1, 2) and np.array_equal(got, want)


@pytest.mark.parametrize("name", ["ds_lifelong", "ds_lifelong_maze"])
def test_episode_goals_on_the_reference_goldens(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    n, T = g["made_actions"].shape
    assert g["lifelong_targets"].shape == (n, 24, 2)
    paths = dt.agent_paths(g["init_positions"], g["made_actions"])
    want = both_restatements(paths, g["lifelong_targets"].tolist())
    assert np.array_equal(dt.episode_goals(g["init_positions"], g["made_actions"], T, g["lifelong_targets"]), want)
    assert (want[:, 1:] != want[:, :-1]).any(-1).sum() >= n                 # the goldens' goals do move


def test_episode_goals_on_random_logs():
    rng = np.random.Generator(np.random.PCG64(11))
    raised = 0
    for _ in range(100):
        n, T, L = int(rng.integers(1, 5)), int(rng.integers(0, 9)), int(rng.integers(1, 6))
        init = rng.integers(15, 25, (n, 2)).astype(np.int16)
        actions = rng.integers(0, 5, (n, T)).astype(np.int8)
        ln = int(rng.integers(0, T + 1))
        paths = lr.paths_of(init, actions, ln)
        # targets: cells of the path (hits) and of its neighbourhood (mostly misses); lists of every length from 1, longer than L too
        targets = np.where(rng.random((n, L, 1)) < 0.6, paths[np.arange(n)[:, None], rng.integers(0, ln + 1, (n, L))],
                           rng.integers(15, 25, (n, L, 2))).astype(np.int16)
        n_targets = rng.integers(1, 2 * L + 2, n) if L > 1 else np.ones(n, np.int64)
        lists = [lr.expand(targets[a], n_targets[a]) for a in range(n)]
        try:
            want = both_restatements(paths, lists)
        except IndexError:
            raised += 1
            with pytest.raises(IndexError):
                dt.episode_goals(init, actions, ln, targets, n_targets)
            continue
        assert np.array_equal(dt.episode_goals(init, actions, ln, targets, n_targets), want)
    assert 10 <= raised <= 90                                                # both ends are exercised


def test_cyclic_addressing_against_an_expanded_list():
    """Q = 2: entry 0, then entries 1, 2, 1, 2, ...; one agent walks right over a row of targets, n_targets beyond 1 + Q."""
    x0, x1 = (5, 6), (5, 7)
    targets = np.array([[x1, x0, x1]], np.int16)                             # target(0) = x1, queue [x0, x1]
    assert lr.expand(targets[0], 6) == [list(x1), list(x0), list(x1), list(x0), list(x1), list(x0)]
    init = np.array([x0], np.int16)
    actions = np.array([[4, 3, 4, 3, 4]], np.int8)                           # x0 x1 x0 x1 x0 x1
    paths = lr.paths_of(init, actions, 5)
    assert paths[0].tolist() == [list(x0), list(x1), list(x0), list(x1), list(x0), list(x1)]
    got = dt.episode_goals(init, actions, 5, targets, [7])
    assert np.array_equal(got, both_restatements(paths, [lr.expand(targets[0], 7)]))
    assert got[0].tolist() == [list(x1), list(x0), list(x1), list(x0), list(x1), list(x0)]     # advances at every step from t = 1; wraps at t = 3
    # the IndexError falls exactly where the expanded list raises: the walk stands on target(t - 1) at every t >= 1, so it needs len + 1
    for n, ln, ok in ((7, 5, True), (6, 5, True), (5, 5, False), (5, 4, True), (3, 5, False), (3, 2, True), (3, 3, False), (1, 0, True),
                      (1, 1, False)):
        lists = [lr.expand(targets[0], n)]
        if ok:
            assert np.array_equal(dt.episode_goals(init, actions, ln, targets, [n]), both_restatements(lr.paths_of(init, actions, ln), lists))
        else:
            with pytest.raises(IndexError):
                dt.goal_positions(lr.paths_of(init, actions, ln), lists)
            with pytest.raises(IndexError):
                dt.episode_goals(init, actions, ln, targets, [n])
    with pytest.raises(IndexError):
        dt.episode_goals(init, actions, 0, targets, [0])                     # an empty list


def test_base_case_data_conditions():
    s = lr.base_case()["stats"]
    assert s == dict(changes=29, at0=18, off_last=127, differ=49), s
    assert s["changes"] >= 20 and s["at0"] >= 5 and s["differ"] >= 1


def test_expected_rows_of_a_plain_list_equal_the_oracle_with_lifelong_targets():
    g = np.load(os.path.join(GOLDEN, "ds_lifelong.npz"))
    n, T = g["made_actions"].shape
    x, y, row0 = lr.expected(g["grid"], g["init_positions"][None], g["made_actions"][None], [T], g["lifelong_targets"][None])
    assert row0.tolist() == [0, n * (T + 1)] and np.array_equal(x.view(np.int8), g["inputs"]) and np.array_equal(y, g["gt_actions"])


# ---- EpisodeStore(lifelong=True) ------------------------------------------------------------------------------------------------------
def test_lifelong_store_grouping_and_name_order_equal_split_by_map_and_files_by_type(tmp_path):
    names = ["zz-random-1", "mazes-b", "aa-random-0", "mazes-a", "plain"]
    rng = np.random.Generator(np.random.PCG64(1))
    batches = [[{"map_name": names[int(rng.integers(0, 5))], "id": 10 * b + k} for k in range(7)] for b in range(3)]
    records = [{"metrics": {}, "env_grid_search": key} for keys in batches for key in keys]
    with open(tmp_path / "log.json", "w") as f:
        json.dump(records, f)
    per_map = db.split_by_map(str(tmp_path / "log.json"), str(tmp_path / "temp"))
    store = db.EpisodeStore(device="cpu", lifelong=True)
    for keys in batches:
        n = len(keys)
        store.add_batch(keys, np.zeros((n, 2, 2), np.int16), np.zeros((n, 2, 3), np.int8), np.full(n, 3, np.int32), np.zeros(n, bool),
                        np.zeros((1, 4, 4), np.uint8), targets=np.zeros((n, 2, 5, 2), np.int16), n_targets=np.ones((n, 2), np.int32))
    assert store.map_names() == list(per_map) and store.episodes() == 21
    assert store.solved_rows() == (21, 21 * 2 * 4)                           # every episode counts, whatever `solved` said
    assert all(tuple(b["targets"].shape) == (7, 2, 5, 2) and tuple(b["n_targets"].shape) == (7, 2) for b in store.batches)
    for name, recs in per_map.items():
        got = [batches[b][k]["id"] for b, idx in store.per_map[name] for k in idx]
        assert got == [r["env_grid_search"]["id"] for r in recs], name
    files = [str(tmp_path / "temp" / f"{n}.json") for n in per_map]
    for chunks in (1, 2):
        want = [([p.rsplit("/", 1)[1] for p in m], [p.rsplit("/", 1)[1] for p in r]) for m, r, _ in db._chunk_plan(files, "x", chunks)]
        got = [(m, r) for m, r, _ in db._chunk_plan([f"{n}.json" for n in store.map_names()], "x", chunks)]
        assert got == want
    with pytest.raises(ValueError, match="targets"):                         # a lifelong store takes no batch without target lists
        store.add_batch(batches[0], np.zeros((7, 2, 2), np.int16), np.zeros((7, 2, 3), np.int8), np.zeros(7, np.int32), np.ones(7, bool),
                        np.zeros((1, 4, 4), np.uint8))
    with pytest.raises(ValueError, match="targets"):                         # ... and a default store none with them
        db.EpisodeStore(device="cpu").add_batch(batches[0], np.zeros((7, 2, 2), np.int16), np.zeros((7, 2, 3), np.int8), np.zeros(7, np.int32),
                                                np.ones(7, bool), np.zeros((1, 4, 4), np.uint8), targets=np.zeros((7, 2, 5, 2), np.int16))


def test_stores_refuse_the_other_kind_of_batch():
    with pytest.raises(NotImplementedError, match="restart"):
        db.EpisodeStore(device="cpu", lifelong=True).append({"on_target": "nothing"})
    with pytest.raises(NotImplementedError, match="restart"):
        db.EpisodeStore(device="cpu", lifelong=True).append({})
    with pytest.raises(NotImplementedError, match="JSON log"):               # as before this section
        db.EpisodeStore(device="cpu").append({"on_target": "restart"})


def test_cli_refusals(tmp_path):
    from mapf_gpt_amd import expert
    cfg = str(tmp_path / "none.yaml")                                        # never opened: the arguments are refused first
    s = str(tmp_path / "s")
    for argv in (["--config", cfg, "--lifelong-shards", s],                                                     # no --desired-size
                 ["--config", cfg, "--lifelong-shards", s, "--desired-size", "10", "--shards", s + "2"],        # two kinds of store
                 ["--config", cfg, "--lifelong-shards", s, "--desired-size", "10", "--algo", "lacam"],          # the search plans no lifelong episode
                 ["--config", cfg, "--shards", s, "--desired-size", "10", "--lifelong"]):                       # still refused
        with pytest.raises(SystemExit) as e:
            expert.main(argv)
        assert e.value.code == 2
    assert not os.path.exists(cfg)


def test_new_symbols_are_bound():
    from mapf_gpt_amd import _lib
    from mapf_gpt_amd.expert import BatchedExpert
    assert "mgpt_dataset_tokenize_episodes_lifelong" in _lib.SYMBOLS
    assert callable(BatchedExpert.lifelong_rows) and callable(BatchedExpert.lifelong_targets) and callable(dt.episode_goals)
    src = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "mapf_gpt_amd.h")).read()
    assert "generate_observations.py:55-60, 72-79, 156-166, 188-202" in src
