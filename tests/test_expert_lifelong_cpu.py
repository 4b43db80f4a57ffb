"""The expert's lifelong mode on the host: hand cases and invariants of the restatement
(tests/expert_lifelong_ref.py), the record format against dataset_tokenizer.goal_positions, the restatement's outcomes on the shapes
tests/test_gpu_expert_lifelong.py compares the device against, and the argument errors that need no device."""
import hashlib

import numpy as np
import pytest

from tests import expert_checks as ec
from tests import expert_lifelong_ref as lr
from tests import expert_ref as er

HAND = lr.hand_cases()


def dist(case, a, frm, to):
    grid = np.asarray(case["grids"])
    return int(er.bfs(grid if grid.ndim == 2 else grid[0], np.asarray(to))[tuple(int(v) for v in frm)])


def arrival_steps(ref, i=0):
    return [t for t, n in enumerate(ref.arrivals[i]) if n]


def test_one_agent_arrives_in_exactly_dist_steps_each_time_and_the_queue_wraps():
    case = HAND["wrap1"]
    ref = lr.run_case(case)
    goals = [case["goal"][0, 0]] + [case["queue"][0, 0, k % 3] for k in range(5)]          # goal, q0, q1, q2, q0, q1
    legs = [dist(case, 0, a, b) for a, b in zip([case["pos"][0, 0]] + goals[:-1], goals)]
    assert legs == [5, 6, 8, 4, 4, 8] and sum(legs) <= case["steps"]
    assert arrival_steps(ref) == (np.cumsum(legs) - 1).tolist()                            # an arrival after leg steps is logged at step leg - 1
    assert ref.reached[0, 0] == 6 and ref.done[0] == 2 and ref.log()[1][0] == case["steps"]
    held = [ref.goal_hist[t][0, 0].tolist() for t in range(case["steps"] + 1)]
    t4 = int(np.cumsum(legs)[3])                                                           # after the fourth arrival: the fourth goal taken
    assert held[t4] == case["queue"][0, 0, 0].tolist() and held[t4 - 1] == case["queue"][0, 0, 2].tolist()      # from the queue is queue[0] again
    assert ref.targets()[0][0] == [g.tolist() for g in goals] + [case["queue"][0, 0, 2].tolist()]


def test_a_next_goal_on_the_agents_own_cell_is_a_second_arrival_on_the_next_steps_wait():
    case = HAND["own_cell"]
    ref = lr.new_ref(case)
    acts = [int(ref.step()[0][0, 0]) for _ in range(3)]
    assert ref.arrivals[0] == [0, 1, 1] and acts[2] == 0                                   # two steps to the goal, then a wait that counts
    assert ref.reached[0, 0] == 2 and ref.since[0, 0] == 0
    assert ref.goal[0, 0].tolist() == case["queue"][0, 0, 1].tolist() and ref.qnext[0, 0] == 2


def test_consecutive_duplicate_queue_entries_count_twice():
    case = HAND["duplicates"]
    ref = lr.run_case(case)
    first = dist(case, 0, case["goal"][0, 0], case["queue"][0, 0, 0])
    assert arrival_steps(ref)[:3] == [1, 1 + first, 2 + first]                             # goal; queue[0]; queue[1] = the same cell, on the wait
    assert ref.made[0][0][2 + first] == 0
    assert [g for g in ref.targets()[0][0][1:3]] == [case["queue"][0, 0, 0].tolist()] * 2


def test_two_agents_with_the_same_goal_cell_arrive_one_after_the_other():
    case = HAND["same_goal2"]
    ref = lr.new_ref(case)
    for t in range(case["steps"]):
        before = ref.goal.copy()
        ref.step()
        on = (ref.pos[0] == before[0]).all(-1)
        assert on.sum() <= 1 or not (before[0, 0] == before[0, 1]).all(), "two agents stand on one cell"
        assert ref.arrivals[0][t] == on.sum()
    assert (ref.reached[0] >= 2).all() and len({tuple(p) for p in ref.pos[0].tolist()}) == 2


def test_in_the_corridor_with_a_pocket_the_order_flips_after_the_first_arrival():
    case = HAND["pocket"]
    ref = lr.new_ref(case)
    assert er.priority_order(ref.since[0]) == [0, 1]
    ref.step()
    ref.step()                                                                             # agent 0 pushes agent 1 into the pocket and arrives
    assert ref.arrivals[0] == [0, 1] and ref.reached[0].tolist() == [1, 0]
    assert ref.since[0].tolist() == [0, 2] and er.priority_order(ref.since[0]) == [1, 0]
    assert ref.goal[0, 0].tolist() == case["queue"][0, 0, 0].tolist()                      # though agent 0 no longer stands on its (new) goal
    act, _ = ref.step()                                                                    # agent 1 plans first: out of the pocket, agent 0 gives way
    assert act[0].tolist() == [3, 1]


SHAPES = [(8, 8, 0.0, 4, 7), (12, 12, 0.2, 8, 7), (16, 16, 0.2, 70, 6), (21, 21, 0.25, 32, 5), (1, 12, 0.0, 3, 4)]


@pytest.mark.parametrize("shape", SHAPES)
def test_every_random_step_keeps_the_invariants_and_the_arrivals_sum_to_reached(shape):
    h, w, density, n_agents, seed = shape
    case = lr.random_case(h, w, density, 3, n_agents, 24, seed=seed, Q=3, n_grids=3)
    ref = lr.new_ref(case)
    for t in range(24):
        before, held = ref.pos.copy(), ref.goal.copy()
        act, planned = ref.step()
        ec.check_transition(case["grids"], before, act, planned, ref.pos, np.zeros(3, bool))
        on = (ref.pos == held).all(-1)
        assert [ref.arrivals[i][t] for i in range(3)] == on.sum(1).tolist()
        assert (ref.since[on] == 0).all() and (ref.since[~on] > 0).all()
    assert (ref.done == 2).all() and (ref.log()[1] == 24).all()                            # truncation only, every log is max_steps long
    assert np.array_equal(ref.arrivals_log().sum(1), ref.reached.sum(1))


def assert_records_mean_what_the_dataset_tokenizer_reads(ref, case):
    from mapf_gpt_amd import dataset_tokenizer as dt
    keys = [{"map_name": "m", "seed": i, "num_agents": case["n_agents"]} for i in range(case["n_inst"])]
    recs = lr.records(ref, keys, case["pos"])
    hist = np.stack(ref.goal_hist)                                                         # [T + 1, inst, agent, 2]
    for i, r in enumerate(recs):
        m = r["metrics"]
        assert set(m) == {"avg_throughput", "ep_length", "made_actions", "init_positions", "global_lifelong_targets_xy"}
        assert m["ep_length"] == case["steps"] and m["avg_throughput"] == float(ref.throughput()[i])
        paths = dt.agent_paths(m["init_positions"], m["made_actions"])
        assert np.array_equal(paths[:, -1], ref.pos[i])
        goals = dt.goal_positions(paths, m["global_lifelong_targets_xy"])
        assert np.array_equal(goals, hist[:, i].transpose(1, 0, 2)), "the logged targets do not reproduce the goals of every step"


@pytest.mark.parametrize("name", ["wrap1", "own_cell", "duplicates", "same_goal2", "pocket", "one_agent", "shared5", "maze8_swap"])
def test_the_records_targets_walk_back_to_the_goal_of_every_step(name):
    case = lr.gpu_cases()[name]
    ref = lr.run_case(case)
    if name == "one_agent":
        assert ref.reached.max() > case["queue"].shape[2] == 2                             # more arrivals than queue entries
    assert_records_mean_what_the_dataset_tokenizer_reads(ref, case)


def test_many_agents_with_a_queue_of_two():
    case = lr.random_case(12, 12, 0.1, 2, 6, 48, seed=4, Q=2)
    ref = lr.run_case(case)
    assert (ref.reached > 2).any()
    assert_records_mean_what_the_dataset_tokenizer_reads(ref, case)


def digest(ref):
    """sha256 over a finished restatement's log, lengths, final positions and goals, reached, since, the arrivals log and throughput."""
    log, lengths = ref.log()
    parts = [(log, np.int8), (lengths, np.int32), (ref.pos, np.int64), (ref.goal, np.int64), (ref.reached, np.int64), (ref.since, np.int64),
             (ref.arrivals_log(), np.int16), (ref.throughput(), np.float32)]
    h = hashlib.sha256()
    for arr, dtype in parts:
        h.update(np.ascontiguousarray(arr, dtype).tobytes())
    return h.hexdigest()


# what the restatement produces on the shapes of tests/test_gpu_expert_lifelong.py: name -> (arrivals per instance, digest(run_case(case)))
OUTCOMES = {
    "wrap1": ([6], "d91b1c7eee0c876960b5f3a28c35ce64530740861ea5a5f1e05ac42de3ebe2df"),
    "own_cell": ([5], "10fe24b953120c758af5a97c2ddfd53b0fc1ef522f86adef0f18a2aefb51087a"),
    "duplicates": ([5], "87f1f1db4727b407436d1dbbfbd2686418566da1b461f1d44ca583c9a6d4df6d"),
    "same_goal2": ([7], "6afddd0d33afdebfecfdd4fbe5e0584fb18f1789b6f580c7e66d75dbe8985aa0"),
    "pocket": ([2], "03c69e27277f7b06cab7822d0480e6b0c6fb9144db8f9d7409fd5708c5649566"),
    "one_agent": ([12], "121fa0a6cf9d6fa8f3c300e0086ff1bb12e21c7ff5ee99e4f59a2c6320cbf122"),
    "agents65": ([111], "71cc58c084c4352748d642c4972efa12861d513a1cb0bda6f69bd0b1b03b44ef"),
    "agents70": ([114], "e0f10293796a8ecde8ab2104d30ed98a8e05eaef088cef9f40b00651447194c7"),
    "grids3": ([30, 31, 35], "2fdc6ff9549fb83d176466d19b5034c886d871cd1ba73ea288aab3acdbd5c936"),
    "shared5": ([31, 32, 36, 29, 25], "db9ac4828857e395cebdb9bd2a92653bc09e03212872c514b18ab6303d63d859"),
    "offset7": ([23, 22, 36], "956a0471403bd668607d745950313dee04ecbcb179cc1df3a13c8abca700b8c1"),
    "maze8_swap": ([12, 13], "0aae24a99d6a033b50d1592fb57c1702317166c899b516f2d60c82937e118579"),
}


def test_the_outcomes_of_the_gpu_shapes_are_pinned():
    cases = lr.gpu_cases()
    assert set(cases) == set(OUTCOMES)
    got = {}
    for name, case in cases.items():
        ref = lr.run_case(case)
        got[name] = (ref.reached.sum(1).tolist(), digest(ref))
    assert got == OUTCOMES


def test_pibt_config_takes_lifelong_and_the_refusals_stay():
    from mapf_gpt_amd import evaluation as ev
    assert ev.PIBTConfig(name="PIBT").lifelong is False
    assert ev.PIBTConfig(name="PIBT", lifelong=True).lifelong is True
    env = {"name": "Environment", "on_target": "restart", "max_episode_steps": 8, "num_agents": 4, "seed": 0,
           "map_name": "validation-random-seed-000"}
    for algo in ({"name": "PIBT", "lifelong": False}, {"name": "LaCAM", "lifelong": True}, {"name": "LaCAM"}):
        with pytest.raises(NotImplementedError, match="lifelong"):
            ev.evaluation({"environment": env, "algorithms": {algo["name"]: algo}}, print_fn=lambda *_: None)


def test_the_evaluations_queue_is_seeded_per_run():
    from mapf_gpt_amd import evaluation as ev, maps
    frame = ev.common_frame([ev.MapRegistry().get("validation-random-seed-000")])[0]
    q = ev.lifelong_queue(frame, 3, 5)
    assert q.shape == (5, ev.LIFELONG_QUEUE, 2) and q.dtype == np.int16
    assert np.array_equal(q, ev.lifelong_queue(frame, 3, 5)) and not np.array_equal(q, ev.lifelong_queue(frame, 4, 5))
    ok = maps.largest_component(frame[0] == 0) & frame[2]
    assert ok[q[..., 0], q[..., 1]].all()


def test_argument_errors_that_need_no_device(monkeypatch):
    from mapf_gpt_amd import expert
    with pytest.raises(ValueError, match="search"):
        expert.BatchedExpert(np.zeros((12, 12), np.uint8), 1, 2, 8, lifelong=True, search="lacam")
    ex = expert.BatchedExpert.__new__(expert.BatchedExpert)                                 # reset()'s own checks come before any device call
    ex.lifelong, ex.n_inst, ex.n_agents, ex._h = True, 2, 3, None
    with pytest.raises(ValueError, match="goal_queue"):
        ex.reset(None, None)
    with pytest.raises(ValueError, match="goal_queue"):
        ex.reset(None, None, goal_queue=np.zeros((2, 3, 4), np.int16))
    with pytest.raises(ValueError, match="goal_queue"):
        ex.reset(None, None, goal_queue=np.zeros((2, 4, 4, 2), np.int16))
    ex.lifelong = False
    with pytest.raises(ValueError, match="lifelong=True"):
        ex.reset(None, None, goal_queue=np.zeros((2, 3, 4, 2), np.int16))
    with pytest.raises(RuntimeError, match="lifelong"):
        ex.targets()


def test_the_cli_refuses_lifelong_with_lacam_and_without_restart(tmp_path, capfd):
    import yaml
    from mapf_gpt_amd import expert
    env = {"name": "Environment", "on_target": "nothing", "max_episode_steps": 8, "num_agents": 4, "seed": 0, "map_name": "validation-random-seed-000"}
    for name, on_target in (("nothing.yaml", "nothing"), ("restart.yaml", "restart")):
        with open(tmp_path / name, "w") as f:
            yaml.safe_dump({"environment": dict(env, on_target=on_target), "algorithms": {}}, f)
    with pytest.raises(SystemExit):
        expert.main(["--config", str(tmp_path / "nothing.yaml"), "--out", str(tmp_path / "o"), "--lifelong"])
    assert "on_target: restart" in capfd.readouterr().err
    with pytest.raises(SystemExit):
        expert.main(["--config", str(tmp_path / "restart.yaml"), "--out", str(tmp_path / "o"), "--lifelong", "--algo", "lacam"])
    assert "--algo lacam" in capfd.readouterr().err
