"""Delta data generation without a device: the library's pick (mapf_gpt_amd.ddg.pick, torch on the host) against
the restatement (tests/ddg_ref.py) on hand tables, `moves` where the env forced a wait, the hand trajectory the device test uses, and
the snapshot / global-id arithmetic under chunking."""
import numpy as np
import pytest
import torch

from mapf_gpt_amd import dataset_tokenizer as dt
from mapf_gpt_amd import ddg
from mapf_gpt_amd.runner import moves_from_positions
from tests import ddg_ref as dr
from tests import expert_ref as er

U = 99          # an unsolved snapshot's cost in the hand tables: above every solved one


def both(valid, solved, cost, min_delta=None):
    """[(picked, j*, delta*)] per instance from the restatement, after checking that the library gives the same."""
    want = dr.pick(valid, solved, cost, min_delta)
    picked, j, d, delta, cand = ddg.pick(torch.tensor(valid), torch.tensor(solved), torch.tensor(cost, dtype=torch.int64), min_delta)
    assert delta.dtype == torch.int64 and j.dtype == torch.int64
    assert [(bool(p), int(a), int(b)) for p, a, b in zip(picked, j, d)] == want
    return want


def test_a_tie_goes_to_the_smaller_j():
    assert both([[True] * 5], [[True] * 5], [[10, 14, 9, 13, 13]]) == [(True, 0, 4)]
    assert both([[True] * 4], [[True] * 4], [[7, 7, 7, 7]]) == [(True, 0, 0)]


def test_an_unsolved_j_is_no_candidate_and_an_unsolved_next_is_the_largest_delta():
    # j = 1 is unsolved: the fall from it (99 -> 12) and everything else about it is ignored as a start, but 0 -> 1 is the largest rise
    assert both([[True] * 4], [[True, False, True, True]], [[20, U, 12, 30]]) == [(True, 0, U - 20)]
    # with j = 0 unsolved too the only candidate is j = 2
    assert both([[True] * 4], [[False, False, True, True]], [[U, U, 12, 30]]) == [(True, 2, 18)]
    # nothing solved: no candidate
    assert both([[True] * 3], [[False] * 3], [[U, U, U]]) == [(False, 0, 0)]
    # the last snapshot is never a start, solved or not
    assert both([[True] * 3], [[False, False, True]], [[U, U, 5]]) == [(False, 0, 0)]


def test_an_episode_shorter_than_k_has_no_candidate():
    T, K = 16, 4
    valid = dr.valid_table([3, 4, 16], T, K)
    assert valid[0] == [True, False, False, False, False] and valid[1] == [True, True, False, False, False]
    assert torch.equal(ddg.snapshot_valid(torch.tensor([3, 4, 16]), T, K), torch.tensor(valid))
    cost = [[9, 0, 0, 0, 0], [9, 11, 0, 0, 0], [9, 11, 8, 30, 2]]
    got = both(valid, [[True] * 5] * 3, cost)
    assert got == [(False, 0, 0), (True, 0, 2), (True, 2, 22)]
    # T < K: one snapshot, no pair
    assert ddg.n_snapshots(3, 4) == 1
    picked, *_ = ddg.pick(torch.tensor([[True]]), torch.tensor([[True]]), torch.tensor([[4]]))
    assert not bool(picked[0])


def test_lengths_exactly_on_a_multiple_of_k():
    T, K = 16, 4
    valid = dr.valid_table([7, 8, 9], T, K)
    assert [sum(v) for v in valid] == [2, 3, 3]                      # t_j <= length: 8 admits snapshot 2, 7 does not
    assert torch.equal(ddg.snapshot_valid(torch.tensor([7, 8, 9]), T, K), torch.tensor(valid))
    cost = [[5, 6, 50, 0, 0]] * 3
    assert both(valid, [[True] * 5] * 3, cost) == [(True, 0, 1), (True, 1, 44), (True, 1, 44)]


@pytest.mark.parametrize("min_delta,want", [(None, True), (-5, True), (3, True), (4, False), (0, True)])
def test_min_delta_on_both_sides_of_the_threshold(min_delta, want):
    got = both([[True] * 3], [[True] * 3], [[10, 13, 11]], min_delta)
    assert got == [(True, 0, 3) if want else (False, 0, 0)]


def test_min_delta_keeps_a_negative_best_only_when_asked():
    assert both([[True] * 3], [[True] * 3], [[10, 8, 3]]) == [(True, 0, -2)]
    assert both([[True] * 3], [[True] * 3], [[10, 8, 3]], 0) == [(False, 0, 0)]


def test_moves_where_the_env_forced_a_wait():
    """Two agents head-on in a corridor ask to swap, a third walks into a wall: the env makes all three wait, the requested actions do
    not reproduce the path, the moves do."""
    grid = er._parse(["#####", "#...#", "#.#.#", "#####"])
    pos = er._cells([(1, 1), (1, 2), (2, 3)])[0]
    made = [[4, 3, 2], [2, 4, 1], [1, 0, 0], [4, 4, 3]]               # [t][agent]
    path = dr.walk(grid, pos, made)
    moves = dr.moves(path)
    assert moves[0][0] == 0 and moves[1][0] == 0 and moves[2][0] == 0          # step 0: swap refused twice, a wall
    assert np.array_equal(dt.agent_paths(pos, moves), path.transpose(1, 0, 2))
    requested = np.asarray(made).T
    assert not np.array_equal(dt.agent_paths(pos, requested), path.transpose(1, 0, 2))
    assert (np.asarray(moves) != requested).any() and (np.asarray(moves) == requested).any()
    # the library's form of it (torch, any device) on [T + 1, inst, agent, 2]
    got = moves_from_positions(torch.from_numpy(path[:, None].astype(np.int16)))
    assert got.dtype == torch.int8 and np.array_equal(got[:, 0].numpy().T, np.asarray(moves))


def test_the_hand_trajectory_picks_the_third_segment():
    h = dr.hand_trajectory()
    path = h["pos_traj"][:, 0]
    dist = np.abs(path - h["goal"][0].astype(np.int64)).sum(-1).sum(-1)         # summed Manhattan distance: falls, falls, rises, falls
    assert dist[0] > dist[4] > dist[8] < dist[12] > dist[16] > 0
    assert ddg.n_snapshots(h["T"], h["every"]) == 5
    for probe in (dict(), dict(swap=True)):
        out = dr.collect(h["grids"], h["pos_traj"], h["lengths"], h["goal"], h["run_keys"], h["every"], probe, ddg.TEACHER)
        assert out["valid"].all() and out["solved"].all() and out["probed"] == 5
        assert out["picked"].tolist() == [True] and out["j"].tolist() == [2] and out["dmax"][0] > 0
        rec, = out["records"]
        assert rec["algorithm"] == "DDG" and rec["metrics"]["CSR"] == 1.0
        assert rec["env_grid_search"] == dict(h["run_keys"][0], ddg_step=8, ddg_delta=int(out["dmax"][0]))
        assert rec["metrics"]["init_positions"] == path[8].tolist()
        end = dt.agent_paths(rec["metrics"]["init_positions"], rec["metrics"]["made_actions"])[:, -1]
        assert np.array_equal(end, h["goal"][0])


def test_snapshot_and_teacher_ids_under_chunking():
    # probe ids g * J + j of three runs g = 4, 5, 9 with 3, 5 and 2 valid snapshots of J = 5: consecutive inside a run, and from run 4
    # to run 5 only if run 4 is complete
    J = 5
    ids = [g * J + j for g, n in ((4, 3), (5, 5), (9, 2)) for j in range(n)]
    assert ids == [20, 21, 22, 25, 26, 27, 28, 29, 45, 46]
    assert ddg.segments(ids, 4096) == [(0, 3), (3, 8), (8, 10)]
    assert ddg.segments(ids, 2) == [(0, 2), (2, 3), (3, 5), (5, 7), (7, 8), (8, 10)]
    assert ddg.segments([5 * J + j for j in range(J)] + [6 * J + j for j in range(J)], 4096) == [(0, 10)]       # complete runs chain
    assert ddg.segments([], 3) == [] and ddg.segments([7], 3) == [(0, 1)]
    for cut in (1, 2, 3, 4096):                       # every id is its segment's first id plus its place in the segment, whatever the cut
        for a, b in ddg.segments(ids, cut):
            assert b - a <= cut and [ids[a] + k for k in range(b - a)] == ids[a:b]
    # teacher ids are the run indices themselves
    assert ddg.segments([4, 5, 9], 4096) == [(0, 2), (2, 3)]
    assert ddg.unsolved_cost(6, 24) == 150 > 6 * 24


def test_a_lifelong_group_is_refused_before_any_device_work():
    h = dr.hand_trajectory()
    with pytest.raises(NotImplementedError, match="joint goal"):
        ddg.collect_from_trajectory(h["grids"], h["pos_traj"], h["lengths"], h["goal"], h["run_keys"], every=4, on_target="restart")
