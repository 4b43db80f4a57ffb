"""The PIBT expert's spec on the host: invariants of every planned step of the restatement (tests/expert_ref.py), the hand cases, the
record schema, and the restatement's solved counts on the shapes tests/test_gpu_expert.py compares the device against."""
import hashlib

import numpy as np
import pytest

from oracle import oracle as orc
from tests import expert_ref as er


def check_step(grid, pos, nxt, act):
    """The invariants of one planned step; returns the cells the oracle's env leaves the agents on."""
    n = len(pos)
    pos = [tuple(int(v) for v in p) for p in pos]
    assert len(set(nxt)) == n, "next cells are not pairwise distinct"
    where = {p: a for a, p in enumerate(pos)}
    for a in range(n):
        assert grid[nxt[a]] == 0, "a blocked cell is planned"
        assert abs(nxt[a][0] - pos[a][0]) + abs(nxt[a][1] - pos[a][1]) <= 1, "more than one cell per move"
        assert nxt[a] == (pos[a][0] + er.MOVES[act[a]][0], pos[a][1] + er.MOVES[act[a]][1])
        b = where.get(nxt[a])
        assert b is None or b == a or nxt[b] != pos[a], "a swap is planned"
    after, _ = orc.env_step(grid, np.asarray(pos), np.zeros((n, 2), np.int32), np.asarray(act, np.int32))      # default rules
    assert [tuple(int(v) for v in p) for p in after] == list(nxt), "the env does not execute the plan as planned"
    return after


@pytest.mark.parametrize("shape", [(8, 8, 0.0, 4, 7), (12, 12, 0.2, 8, 7), (16, 16, 0.2, 70, 6), (21, 21, 0.25, 32, 5), (1, 12, 0.0, 3, 4)])
def test_every_random_step_keeps_the_invariants(shape):
    h, w, density, n_agents, seed = shape
    case = er.random_case(h, w, density, 3, n_agents, 24, seed=seed, n_grids=3)
    ref = er.RefExpert(case["grids"], 3, n_agents, 24, seed)
    ref.reset(case["pos"], case["goal"])
    for t in range(24):
        for i in range(3):
            if ref.done[i]:
                continue
            nxt, act, _ = er.plan(ref.grid(i), ref.pos[i], ref.dist[i], ref.since[i], ref.seed, ref.t, i * n_agents)
            check_step(ref.grid(i), ref.pos[i], nxt, act)
        before = ref.pos.copy()
        _, planned = ref.step()
        assert np.array_equal(ref.pos, planned), "the restatement's own env left an agent off its planned cell"
        assert (np.abs(ref.pos - before).sum(-1) <= 1).all()


def test_the_restatements_env_is_the_oracles():
    rng = np.random.default_rng(0)
    case = er.random_case(12, 12, 0.2, 1, 10, 1, seed=0)
    grid, pos = case["grids"][0], case["pos"][0]
    for _ in range(50):
        act = rng.integers(0, 5, 10)
        want, _ = orc.env_step(grid, pos, case["goal"][0], act)
        got = np.asarray(er.env_step(grid, pos, act))
        assert np.array_equal(got, want)
        pos = got


def test_bfs_is_the_oracles():
    case = er.random_case(16, 16, 0.25, 1, 4, 1, seed=0)
    for a in range(4):
        assert np.array_equal(er.bfs(case["grids"][0], case["goal"][0, a]), orc.bfs(case["grids"][0], case["goal"][0, a]))


def test_one_agent_arrives_in_exactly_dist_steps():
    case = er.gpu_cases()["one_agent"]
    d = int(er.bfs(case["grids"][0], case["goal"][0, 0])[tuple(case["pos"][0, 0])])
    assert 0 < d < case["steps"]
    ref = er.run_case(case)
    m = ref.metrics()[0]
    assert m[0] == 1.0 and m[4] == d and ref.done[0] == 1 and ref.log()[1][0] == d


def test_head_on_in_a_corridor_pushes_the_lower_priority_agent_into_the_pocket():
    case = er.hand_cases()["pocket"]
    ref = er.run_case(case, steps=0)
    a0, p0 = ref.step()                                          # agent 0 advances, agent 1 finds its best cell reserved and waits
    assert a0[0].tolist() == [4, 0]
    a1, p1 = ref.step()                                          # agent 0 wants agent 1's cell: inheritance, and the only way out is down
    assert a1[0].tolist() == [4, 2]
    assert p1[0, 1].tolist() == [2 + er.PAD, 3 + er.PAD] and p1[0, 0].tolist() == case["goal"][0, 0].tolist()
    assert ref.max_depth == 2
    assert np.array_equal(ref.pos[0], p1[0])


def test_three_agents_on_a_block_rotate():
    case = er.hand_cases()["rotation"]
    ref = er.run_case(case, steps=0)
    act, planned = ref.step()
    assert act[0].tolist() == [4, 2, 3] and ref.max_depth == 3
    assert np.array_equal(planned[0], case["goal"][0]) and np.array_equal(ref.pos[0], case["goal"][0])
    assert ref.done[0] == 1 and ref.metrics()[0, 4] == 1


def test_full_dead_end_reaches_depth_eight_and_unwinds_to_a_wait():
    case = er.hand_cases()["dead_end"]
    ref = er.run_case(case, steps=0)
    act, planned = ref.step()
    assert ref.max_depth == 8
    assert act[0].tolist() == [0] * 8 and np.array_equal(planned[0], case["pos"][0])


def test_priority_order_with_since_ties():
    assert er.priority_order([3, 0, 3, 1]) == [0, 2, 3, 1]
    assert er.priority_order([0, 0, 0]) == [0, 1, 2]
    assert er.priority_order([1, 2, 2, 1, 5]) == [4, 1, 2, 0, 3]
    # an agent off its goal overtakes the ones standing on theirs: after one step agent 1 (off goal) plans before agent 0 (on goal)
    grid = er._parse(["#####", "#...#", "#####"])
    ref = er.RefExpert(grid, 1, 2, 8, seed=0)
    ref.reset(er._cells([(1, 1), (1, 3)]), er._cells([(1, 1), (1, 2)]))
    assert ref.since[0].tolist() == [0, 0]                       # 0 at reset, on the goal or not
    ref2 = er.RefExpert(grid, 1, 2, 8, seed=0)
    ref2.reset(er._cells([(1, 2), (1, 3)]), er._cells([(1, 2), (1, 1)]))
    ref2.step()                                                  # agent 0 (first by id) waits on its goal, agent 1 is blocked by it
    assert ref2.since[0].tolist() == [0, 1]
    act, _ = ref2.step()                                         # now agent 1 is first: it pushes agent 0 off its goal
    assert act[0].tolist() == [3, 3]


def test_records_go_through_the_dataset_tokenizers_host_side():
    from mapf_gpt_amd import dataset_tokenizer as dt
    case = er.gpu_cases()["shared5"]
    ref = er.run_case(case)
    keys = [{"map_name": "m", "seed": i, "num_agents": case["n_agents"]} for i in range(case["n_inst"])]
    recs = er.records(ref, keys, case["pos"])
    assert len(recs) == case["n_inst"]
    for i, r in enumerate(recs):
        assert set(r) == {"metrics", "env_grid_search", "algorithm"} and r["algorithm"] == "PIBT"
        m = r["metrics"]
        assert set(m) == {"CSR", "ISR", "SoC", "makespan", "ep_length", "avg_agents_density", "made_actions", "init_positions"}
        T = int(m["ep_length"])
        assert len(m["made_actions"]) == case["n_agents"] and all(len(a) == T for a in m["made_actions"])
        paths = dt.agent_paths(m["init_positions"], m["made_actions"])
        labels = dt.gt_actions(m["made_actions"])
        assert paths.shape == (case["n_agents"], T + 1, 2) and all(len(g) == T + 1 for g in labels)
        assert np.array_equal(paths[:, -1], ref.pos[i]), "the logged actions do not lead to the final cells"
        if m["CSR"] == 1.0:
            assert np.array_equal(paths[:, -1], case["goal"][i])


# what the restatement produces on the shapes of tests/test_gpu_expert.py (the device must equal it case by case; no share of solved
# episodes is a bar anywhere): name -> (solved instances, instances)
SOLVED = {"pocket": (0, 1), "rotation": (1, 1), "dead_end": (0, 1), "one_agent": (1, 1), "agents65": (0, 1), "agents70": (0, 1),
          "grids3": (3, 3), "shared5": (4, 5), "empty32": (32, 32), "offset7": (3, 3)}


def test_solved_counts_of_the_gpu_shapes():
    cases = er.gpu_cases()
    assert set(cases) == set(SOLVED)
    got = {}
    for name, case in cases.items():
        ref = er.run_case(case)
        got[name] = (int(ref.metrics()[:, 0].sum()), case["n_inst"])
    assert got == SOLVED


def digest(ref):
    """sha256 over a finished restatement's log, lengths, final positions, done flags and metrics, and,
    where it searched, over status, iterations, nodes, length and every solution."""
    log, lengths = ref.log()
    parts = [(log, np.int8), (lengths, np.int32), (ref.pos, np.int64), (ref.done, np.uint8), (ref.metrics(), np.float64)]
    if hasattr(ref, "found"):
        parts += [(s, np.int32) for s in ref.stats()]
        parts += [(f["solution"], np.int8) for f in ref.found if f["solution"] is not None]
    h = hashlib.sha256()
    for arr, dtype in parts:
        h.update(np.ascontiguousarray(arr, dtype).tobytes())
    return h.hexdigest()


# The three restatements once held four copies of the generator, two of the search and three of the episode step.  These digests (and
# those of tests/test_expert_search_cpu.py and tests/test_expert_swap_cpu.py) were computed with that code, on every case and mode,
# before the copies were folded into expert_ref.gen, expert_search_ref.search and RefExpert.plan_instance: name -> digest(run_case(case))
DIGESTS = {
    "agents65": "13278d0db10a4909922173c599b6846bc1937be7af2d917d156f98747c8515e5",
    "agents70": "f3f8fb4d77b1aa11c57fdf32dc5f5d779e4cc31f692c30693f8ac7ba8c458fee",
    "dead_end": "e4ad371d0863106482f2143dae3b48cde24b77ecf7dc2603733460c285541c18",
    "empty32": "a34b4d0cb2818e427999733db95dc61f26fad075903540fbb08710838ca3c20b",
    "grids3": "bda730317c520112eb9a3b200fc2740b309d3c83a0b5bd962281363293fbeb68",
    "offset7": "7ff9eb94b377d3862e0fd0dc93947015989b131f7534f9f856d3b472d0299479",
    "one_agent": "8ea4d162561388b8d808b7ba214d0dd26f03ca388f1d03f047eb30c273cbdcf9",
    "pocket": "74f400dd2d16e04fc3349ec6ad42f63404151396d68388ba1639d7315038c22f",
    "rotation": "4d169063e2b52792a2e1bf65a51733510d2951d58bdae06e2612182b9d9159d5",
    "shared5": "8f580042702ab7131c72494830c6c9c41a55ffae01678a51f3359957ebbf15b1",
}


def test_the_episodes_of_the_gpu_shapes_are_bit_for_bit_what_they_were():
    cases = er.gpu_cases()
    assert set(cases) == set(DIGESTS)
    assert {name: digest(er.run_case(case)) for name, case in cases.items()} == DIGESTS


def test_evaluation_refuses_what_the_pibt_branch_does_not_build():
    from mapf_gpt_amd import evaluation as ev
    env = {"name": "Environment", "on_target": "restart", "max_episode_steps": 8, "num_agents": 4, "seed": 0,
           "map_name": "validation-random-seed-000"}
    cfg = {"environment": env, "algorithms": {"PIBT": {"name": "PIBT", "seed": 1}}}
    with pytest.raises(NotImplementedError, match="lifelong"):
        ev.evaluation(cfg, print_fn=lambda *_: None)
    cfg["environment"] = dict(env, on_target="nothing")
    with pytest.raises(ValueError, match="world == 1"):
        ev.evaluation(cfg, print_fn=lambda *_: None, log_actions=True, rank=0, world=2)
    with pytest.raises(TypeError):
        ev.PIBTConfig(name="PIBT", batch_size=4)               # unknown keys raise
    c = ev.PIBTConfig(name="PIBT", seed=None)
    assert (c.name, c.seed, c.device) == ("PIBT", 0, "cuda")
