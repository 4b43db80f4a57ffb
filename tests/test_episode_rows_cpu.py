"""Host side of the batched episode tokenizer: the offsets and label rules as numpy states them, the store's
grouping against split_by_map, the frame-fill invariance through the restatement, the table cache and the CLI refusals.  No device."""
import json

import numpy as np
import pytest
import torch

from mapf_gpt_amd import dataset_build as db
from mapf_gpt_amd import dataset_tokenizer as dt
from mapf_gpt_amd import maps
from tests import episode_rows_ref as rr


@pytest.mark.parametrize("keep,want", [
    (None, [0, 21, 27, 30, 42, 63]),
    ([0, 1, 1, 1, 1], [0, 0, 6, 9, 21, 42]),                # first skipped
    ([1, 1, 0, 1, 1], [0, 21, 27, 27, 39, 60]),             # middle
    ([1, 1, 1, 1, 0], [0, 21, 27, 30, 42, 42]),             # last
    ([0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]),                  # all
])
def test_offsets_against_hand_tables(keep, want):
    # 3 agents, cap 6: lengths 6 (= the cap), 1, 0, 3 and 9 (beyond the cap: counts as 6) give 21, 6, 3, 12, 21 rows
    assert dt.episode_row_offsets([6, 1, 0, 3, 9], 3, 6, keep).tolist() == want


def test_offsets_follow_the_selection_and_clamp_below_zero():
    assert dt.episode_row_offsets([6, 1, 0, 3, 9], 3, 6, [1, 0, 1, 1, 1], episodes=[4, 1, 0, 4]).tolist() == [0, 21, 21, 42, 63]
    assert dt.episode_row_offsets([-2, 2], 5, 4).tolist() == [0, 5, 20]
    assert dt.episode_row_offsets([], 5, 4).tolist() == [0]
    assert dt.episode_row_offsets([3, 3], 2, 4, episodes=[]).tolist() == [0]


def test_label_rule_equals_gt_actions():
    hand = np.array([[0, 0, 0, 0],          # an all-wait agent: no 5 anywhere
                     [0, 0, 0, 3],          # a move in the last slot: only the appended wait becomes 5
                     [1, 2, 0, 0],          # trailing waits
                     [0, 4, 0, 1]], np.int8)
    assert dt.episode_labels(hand, 4).tolist() == [[0, 0, 0, 0, 0], [0, 0, 0, 3, 5], [1, 2, 5, 5, 5], [0, 4, 0, 1, 5]]
    assert dt.episode_labels(hand, 4).tolist() == dt.gt_actions(hand.tolist())
    assert dt.episode_labels(hand, 2).tolist() == dt.gt_actions(hand[:, :2].tolist()) == [[0, 0, 0], [0, 0, 0], [1, 2, 5], [0, 4, 5]]
    assert dt.episode_labels(hand, 0).tolist() == [[0]] * 4
    rng = np.random.Generator(np.random.PCG64(3))
    for _ in range(100):
        n, T = int(rng.integers(1, 5)), int(rng.integers(0, 9))
        a = (rng.integers(0, 5, (n, T)) * (rng.random((n, T)) < 0.5)).astype(np.int8)
        L = int(rng.integers(0, T + 1))
        assert dt.episode_labels(a, L).tolist() == dt.gt_actions([r[:L].tolist() for r in a])
    bad = np.array([[9, 1, -3, 0]], np.int8)                # bytes outside 0..4 count as waits
    assert dt.episode_labels(bad, 4).tolist() == [[0, 1, 5, 5, 5]]


def test_store_grouping_and_name_order_equal_split_by_map_and_files_by_type(tmp_path):
    names = ["zz-random-1", "mazes-b", "aa-random-0", "mazes-a", "plain"]
    rng = np.random.Generator(np.random.PCG64(0))
    batches = [[{"map_name": names[int(rng.integers(0, 5))], "id": 10 * b + k} for k in range(7)] for b in range(3)]
    records = [{"metrics": {}, "env_grid_search": key} for keys in batches for key in keys]
    with open(tmp_path / "log.json", "w") as f:
        json.dump(records, f)
    per_map = db.split_by_map(str(tmp_path / "log.json"), str(tmp_path / "temp"))
    store = db.EpisodeStore(device="cpu")
    for keys in batches:
        n = len(keys)
        store.add_batch(keys, np.zeros((n, 2, 2), np.int16), np.zeros((n, 2, 3), np.int8), np.zeros(n, np.int32), np.ones(n, bool),
                        np.zeros((1, 4, 4), np.uint8))
    assert store.map_names() == list(per_map) and store.episodes() == 21
    for name, recs in per_map.items():
        got = [batches[b][k]["id"] for b, idx in store.per_map[name] for k in idx]
        assert got == [r["env_grid_search"]["id"] for r in recs], name
    files = [str(tmp_path / "temp" / f"{n}.json") for n in per_map]
    for chunks in (1, 2):
        want = [([p.rsplit("/", 1)[1] for p in m], [p.rsplit("/", 1)[1] for p in r]) for m, r, _ in db._chunk_plan(files, "x", chunks)]
        got = [(m, r) for m, r, _ in db._chunk_plan([f"{n}.json" for n in store.map_names()], "x", chunks)]
        assert got == want
    mz, rd = db.files_by_type(files)
    assert [p.rsplit("/", 1)[1] for p in mz] == ["mazes-a.json", "mazes-b.json"] and len(rd) == 2


def test_store_refuses_a_lifelong_batch():
    with pytest.raises(NotImplementedError, match="JSON log"):
        db.EpisodeStore(device="cpu").append({"on_target": "restart"})


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_a_larger_frame_changes_no_row(seed):
    """The table is built from the expert's frame grid: blocked fill around the map's own padded grid is unreachable for the table
    and a wall for the window, so rows and labels are those of the map's own grid."""
    obst = maps.random_map(9, 11, 0.2, 50 + seed)
    own = maps.pad(obst)
    frame = np.ones((own.shape[0] + 4, own.shape[1] + 7), np.uint8)
    frame[:own.shape[0], :own.shape[1]] = own
    init, actions = rr.random_walks(own, 1, 7, 6, [6], seed)
    made = [a.tolist() for a in actions[0]]
    from oracle import dataset_oracle as dso
    x0, y0 = dso.generate_observations(own, init[0].astype(int).tolist(), made)
    x1, y1 = dso.generate_observations(frame, init[0].astype(int).tolist(), made)
    assert np.array_equal(x0, x1) and np.array_equal(y0, y1) and len(x0) == 7 * 7


def test_table_cache_budget_and_oldest_first_eviction():
    made = []

    def make(grid, device):
        made.append(grid.copy())
        return object()

    g = [np.zeros((4, 4), np.uint8) for _ in range(4)]
    for k in range(4):
        g[k][0, k] = 1
    size = 2 * 16 * 16
    cache = dt.TableCache(budget_bytes=2 * size, device="cpu", make=make)
    a, b = cache.get(g[0]), cache.get(g[1])
    assert cache.get(g[0] * 7) is a and cache.get(torch.as_tensor(g[1])) is b and cache.builds == 2      # the key is blocked / free
    c = cache.get(g[2])                                     # over the budget: the oldest table leaves
    assert len(cache) == 2 and cache.bytes == 2 * size and cache.get(g[1]) is b and cache.get(g[2]) is c and cache.builds == 3
    assert cache.get(g[0]) is not a and cache.builds == 4 and len(cache) == 2
    tall = np.zeros((8, 4), np.uint8)                       # same bytes as a 4 x 8 grid, another shape: another table
    small = dt.TableCache(budget_bytes=1, device="cpu", make=make)
    t1 = small.get(tall)
    assert len(small) == 1 and small.get(tall) is t1        # the newest stays even when it alone exceeds the budget
    assert small.get(tall.reshape(4, 8)) is not t1 and len(small) == 1


def test_cli_refusals(tmp_path):
    from mapf_gpt_amd import ddg, expert
    cfg = str(tmp_path / "none.yaml")                       # never opened: the arguments are refused first
    for argv in (["--config", cfg],                                                             # neither --out nor --shards
                 ["--config", cfg, "--shards", str(tmp_path / "s")],                           # no --desired-size
                 ["--config", cfg, "--shards", str(tmp_path / "s"), "--desired-size", "10", "--lifelong"]):
        with pytest.raises(SystemExit) as e:
            expert.main(argv)
        assert e.value.code == 2
    for argv in (["--weights", "synthetic:tiny", "--config", cfg],
                 ["--weights", "synthetic:tiny", "--config", cfg, "--shards", str(tmp_path / "s")]):
        with pytest.raises(SystemExit) as e:
            ddg.main(argv)
        assert e.value.code == 2


def test_new_symbols_are_bound():
    from mapf_gpt_amd import _lib
    assert {"mgpt_dataset_episode_offsets", "mgpt_dataset_tokenize_episodes"} <= set(_lib.SYMBOLS)
    from mapf_gpt_amd.expert import BatchedExpert
    assert callable(BatchedExpert.dataset_rows) and callable(db.build_shards_from_store) and callable(dt.tokenize_episodes)
