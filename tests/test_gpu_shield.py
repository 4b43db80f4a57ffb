"""The collision shield on the device against its restatement (tests/shield_ref.py): the standalone planner with
seeded logits and `first` on the smallest shapes at which the kernel can go wrong, property 2 on the device, the shield behind the policy
in BatchedRunner (graph, retire mode, shards, determinism, shield=None), the refusals of the C ABI and the evaluation's metric."""
import os

import numpy as np
import pytest

from tests import expert_checks as ck
from tests import expert_ref as er
from tests import shield_ref as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 24


def _corridor():
    grids = er._parse(["#######", "#.....#", "#######"])
    return dict(grids=grids, n_inst=1, n_agents=3, pos=er._cells([(1, 1), (1, 3), (1, 4)]), goal=er._cells([(1, 5), (1, 1), (1, 2)]),
                steps=STEPS, seed=2, inst_offset=0)


CASES = {
    "one_agent": er.random_case(12, 12, 0.2, 1, 1, STEPS, seed=1),
    "corridor3": _corridor(),                                            # 3 agents in a 1 x 5 corridor
    "agents8": er.random_case(12, 12, 0.2, 1, 8, STEPS, seed=3),
    "agents65": er.random_case(12, 12, 0.0, 1, 65, STEPS, seed=4),       # past one wave's lanes
    "agents70": er.random_case(16, 16, 0.2, 1, 70, STEPS, seed=5),
    "grids2": er.random_case(12, 12, 0.2, 4, 8, STEPS, seed=6, n_grids=2),      # inst % n_grids
}


def make_shield(case, steps=None):
    import torch
    from mapf_gpt_amd.expert import BatchedExpert
    ex = BatchedExpert(case["grids"], case["n_inst"], case["n_agents"], steps or case["steps"], shield=True)
    ex.reset(torch.from_numpy(case["pos"]), torch.from_numpy(case["goal"]))
    ref = sr.RefShield(case["grids"], case["n_inst"], case["n_agents"], steps or case["steps"])
    ref.reset(case["pos"], case["goal"])
    return ex, ref


def device_step(ex, bits, first, width=5):
    """One shield_step with the logits given as bit patterns [inst, agent, width] -> (actions, planned, pos, done, overrides) as numpy."""
    import torch
    logits = torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32).reshape(-1, width))
    act = ex.shield_step(logits, torch.from_numpy(np.asarray(first, np.int32))).cpu().numpy().copy()
    pos, _, done = ex.env.sync_state()
    return act, ex.planned().cpu().numpy(), pos.cpu().numpy(), done.cpu().numpy(), ex.shield_overrides().cpu().numpy()


def assert_step(got, want_actions, want_planned, ref, skip, t):
    act, planned, pos, done, over = got
    live = ~skip
    assert np.array_equal(act, want_actions), f"actions differ at step {t}"          # (a skipped instance keeps `first`)
    assert np.array_equal(planned[live], want_planned[live]), f"planned cells differ at step {t}"
    assert np.array_equal(pos, ref.pos), f"env positions differ at step {t}"
    assert np.array_equal(done, ref.done), f"done flags differ at step {t}"
    assert np.array_equal(over, ref.overrides), f"overrides differ at step {t}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_step_equals_the_restatement(name):
    case = CASES[name]
    n_inst, n = case["n_inst"], case["n_agents"]
    ex, ref = make_shield(case)
    rng = np.random.default_rng(case["seed"])
    for t in range(STEPS):
        width = 5 if t % 2 else 7                                        # ld > 5: only the first five values of a row are read
        bits = sr.random_logits(rng, n_inst, n, width)
        first = rng.integers(0, 5, size=(n_inst, n))
        before, skip = ref.pos.copy(), ref.done != 0
        want = ref.step(bits, first)                                      # since feeds the next step's order: its effects show there
        got = device_step(ex, bits, first, width)
        assert_step(got, *want, ref, skip, t)
        assert np.array_equal(ex.shield_first().cpu().numpy()[~skip], first[~skip])
        ck.check_transition(case["grids"], before, np.where(skip[:, None], 0, got[0]), np.where(skip[:, None, None], before, got[1]), got[2], skip)
    assert ref.overrides.sum() > 0 or n == 1


def test_the_hand_bit_patterns_as_logits():
    """One agent in the middle of an open block (every action a candidate), or with a wall above it: `first` is tried first, so the
    planned action is the head of the expected order; with `first` withheld (an action outside 0..4) it is the best by the logits."""
    open_grid, wall_grid = er._parse(["...", "...", "..."]), er._parse(["###", "...", "..."])
    for name, (bits, first, cand, order) in sorted(sr.hand_patterns().items()):
        grid = open_grid if len(cand) == 5 else wall_grid
        case = dict(grids=grid, n_inst=1, n_agents=1, pos=er._cells([(1, 1)]), goal=er._cells([(2, 2)]), steps=4)
        for f, want in ((first, order[0]), (-1, sr.preference(cand, -1, bits)[0])):
            ex, ref = make_shield(case)
            skip = ref.done != 0
            exp = ref.step(np.array(bits, np.uint32).reshape(1, 1, 5), np.array([[f]]))
            assert exp[0][0, 0] == want, name
            assert_step(device_step(ex, np.array(bits, np.uint32).reshape(1, 1, 5), [[f]]), *exp, ref, skip, name)


WAIT_BITS = [sr.TWO, sr.ONE, sr.ONE, sr.ONE, sr.ONE]                      # a blocker's logits: it prefers to wait


def _blocked_scenarios():
    """The whole preference order on the device: agent 4 (lowest priority at reset) stands at (1, 1) of an open block with the hand
    pattern as its logits, and agents 0..3 wait on the cells of its best j moves (the others are parked out of reach), so it has to take
    its next choice.  `pushed`: the next agent stands on the cell of agent 4's LAST move and steps into (1, 1), so agent 4 is called by
    inheritance and can neither wait nor take that agent's cell.
    -> per grid name: list of (pattern name, positions [5][2], first [5], bits [5][5], the action agent 4 must take or None)."""
    park = [(3, 0), (3, 1), (3, 2), (4, 0)]
    out = {"open": [], "wall": []}
    for name, (bits, first, cand, order) in sorted(sr.hand_patterns().items()):
        moves = [k for k in order if k != 0]
        for pushed in (False, True):
            for j in range(len(moves) + (0 if pushed else 1)):
                blocked = moves[:j]
                pos, fst = list(park), [0, 0, 0, 0, first]
                for i, k in enumerate(blocked):
                    pos[i] = (1 + er.MOVES[k][0], 1 + er.MOVES[k][1])
                if pushed:
                    k = moves[-1]
                    if k in blocked:
                        continue
                    pos[j] = (1 + er.MOVES[k][0], 1 + er.MOVES[k][1])         # after the waiters in the order: they are decided
                    fst[j] = {1: 2, 2: 1, 3: 4, 4: 3}[k]                      # towards (1, 1)
                    blocked = blocked + [0, k]
                want = next((k for k in order if k not in blocked), None)
                out["open" if len(cand) == 5 else "wall"].append((name, pos + [(1, 1)], fst, [WAIT_BITS] * 4 + [list(bits)], want))
    return out


@pytest.mark.parametrize("which", ["open", "wall"])
def test_the_whole_preference_order_on_hand_bit_patterns(which):
    """Every scenario is one instance of one context, one step each: the device equals the restatement, and agent 4 takes the first
    action of the expected order that the others leave it."""
    rows = {"open": ["...", "...", "...", "...", "..."], "wall": ["###", "...", "...", "...", "..."]}[which]
    scen = _blocked_scenarios()[which]
    assert len(scen) >= 7                                                 # (the wall pattern has three moves: 4 + 3 scenarios)
    pos = np.stack([er._cells(p)[0] for _, p, _, _, _ in scen])
    goal = pos.copy()
    goal[:, 4] = er._cells([(4, 2)])[0, 0]                               # the blockers rest on their goals; agent 4 has somewhere to go
    case = dict(grids=er._parse(rows), n_inst=len(scen), n_agents=5, pos=pos, goal=goal, steps=4)
    ex, ref = make_shield(case)
    bits = np.array([b for _, _, _, b, _ in scen], np.uint32)
    first = np.array([f for _, _, f, _, _ in scen])
    skip = ref.done != 0
    want = ref.step(bits, first)
    seen = set()
    for i, (name, _, _, _, must) in enumerate(scen):
        if must is not None:
            assert want[0][i, 4] == must, (name, i)
            seen.add((name, sr.hand_patterns()[name][3].index(must)))
    assert_step(device_step(ex, bits, first), *want, ref, skip, which)
    if which == "open":                                                   # every place of every five-candidate order was forced at least once
        assert {r for _, r in seen} == {0, 1, 2, 3, 4}


def _live_step(ex, ref, live, bits, first, t):
    """One mgpt_expert_shield call with the live list `live` (ids in any order) and compact logits, then env step and commit; the
    instances outside the list get all-wait actions from the caller.  The restatement takes the same list through step(live=)."""
    import torch
    from mapf_gpt_amd import _lib
    n_inst, n = ref.n_inst, ref.n_agents
    others = [i for i in range(n_inst) if i not in live]
    first = first.copy()
    first[others] = 0
    compact = np.zeros((n_inst, n, 5), np.uint32)
    compact[:len(live)] = bits[live]                                      # compact row block b = instance live[b]
    compact[len(live):] = sr.QNAN                                         # (never read: beyond the count)
    d_logits = torch.from_numpy(compact.view(np.float32).reshape(-1, 5)).cuda()
    d_live = torch.from_numpy(np.array(list(live) + [-1] * (n_inst - len(live)), np.int32)).cuda()
    d_count = torch.tensor([len(live)], dtype=torch.int32, device="cuda")
    planned_before, first_before = ex.planned().cpu().numpy(), ex.shield_first().cpu().numpy()
    ex.actions.copy_(torch.from_numpy(first.astype(np.int32)))
    L, s = _lib.lib(), _lib.stream_ptr()
    _lib.check(L.mgpt_expert_shield(ex._h, _lib.ptr(d_logits), 5, _lib.ptr(d_live), _lib.ptr(d_count), _lib.ptr(ex.actions.view(-1)), s))
    _lib.check(L.mgpt_env_step(ex.env._h, _lib.ptr(ex.actions.view(-1)), s))
    _lib.check(L.mgpt_expert_shield_commit(ex._h, s))
    skip = ref.done != 0
    handled = np.array([i in live and not skip[i] for i in range(n_inst)])
    want_act, want_planned = ref.step(bits, first, live=list(live))
    ref.step(bits, first, live=others)                                    # all-wait is collision-free: it comes back unchanged (property 2)
    pos, _, done = ex.env.sync_state()
    act, planned = ex.actions.cpu().numpy(), ex.planned().cpu().numpy()
    assert np.array_equal(act, want_act), f"actions differ at step {t}"
    assert np.array_equal(planned[handled], want_planned[handled]), f"planned cells differ at step {t}"
    assert np.array_equal(planned[~handled], planned_before[~handled]), f"an instance outside the list was planned at step {t}"
    assert np.array_equal(ex.shield_first().cpu().numpy()[~handled], first_before[~handled]), t
    assert np.array_equal(ex.shield_first().cpu().numpy()[handled], first[handled]), t
    assert np.array_equal(pos.cpu().numpy(), ref.pos) and np.array_equal(done.cpu().numpy(), ref.done), t
    assert np.array_equal(ex.shield_overrides().cpu().numpy(), ref.overrides), t


def test_a_permuted_shortened_live_list_with_compact_logits():
    """The live-list branch of the kernel by hand: block b handles instance live[b] with the logits of compact row block b, actions and
    positions stay at the global rows, blocks beyond the count and instances outside the list do nothing."""
    case = er.random_case(12, 12, 0.2, 5, 8, STEPS, seed=8)
    ex, ref = make_shield(case)
    rng = np.random.default_rng(8)
    lists = [[3, 0, 4], [4, 3, 0, 1], [2], [], [1, 4, 2, 0, 3], [0, 3], [4, 1, 2], [3, 0, 4]]
    for t, live in enumerate(lists):
        _live_step(ex, ref, live, sr.random_logits(rng, 5, 8), rng.integers(0, 5, size=(5, 8)), t)
    assert ref.overrides.min() > 0 and (ref.pos != case["pos"]).any()


def test_an_instance_that_finishes_early_is_left_untouched():
    """Instance 0: one step from its goals, done after the first step; instance 1 runs on.  Afterwards instance 0's actions keep whatever
    the caller wrote, its planned cells, positions and counter stay."""
    grid = er._parse(["....", "....", "....", "...."])
    pos = np.stack([er._cells([(0, 0), (3, 3)])[0], er._cells([(0, 0), (0, 3)])[0]])
    goal = np.stack([er._cells([(0, 1), (3, 2)])[0], er._cells([(3, 3), (3, 0)])[0]])
    case = dict(grids=grid, n_inst=2, n_agents=2, pos=pos, goal=goal, steps=8)
    ex, ref = make_shield(case)
    rng = np.random.default_rng(0)
    first = np.array([[4, 3], [2, 2]])
    for t in range(4):
        bits = sr.random_logits(rng, 2, 2)
        skip = ref.done != 0
        want = ref.step(bits, first)
        got = device_step(ex, bits, first)
        assert_step(got, *want, ref, skip, t)
        if t == 0:
            assert ref.done.tolist() == [1, 0]
            planned0, over0 = got[1][0].copy(), got[4][0]
        else:
            assert np.array_equal(got[0][0], first[0]) and np.array_equal(got[1][0], planned0) and got[4][0] == over0
        first = rng.integers(0, 5, size=(2, 2))


def test_a_collision_free_joint_action_comes_back_unchanged():
    """Property 2 on the device: the restatement's own plan (for other logits) fed back as `first`, with arbitrary logits."""
    case = CASES["agents70"]
    n_inst, n = case["n_inst"], case["n_agents"]
    ex, ref = make_shield(case)
    rng = np.random.default_rng(9)
    for t in range(8):
        first = np.stack([sr.plan(ref.grid(i), ref.pos[i], ref.dist[i], ref.since[i], rng.integers(0, 5, size=n), sr.random_logits(rng, 1, n)[0])[1]
                          for i in range(n_inst)])
        assert all(sr.is_collision_free(ref.grid(i), ref.pos[i], ref.dist[i], first[i]) for i in range(n_inst))
        bits = sr.random_logits(rng, n_inst, n)
        skip = ref.done != 0
        want = ref.step(bits, first)
        got = device_step(ex, bits, first)
        assert_step(got, *want, ref, skip, t)
        assert np.array_equal(got[0], first) and (got[4] == 0).all()
    assert (ref.pos != case["pos"]).any()


# ---- through the policy ---------------------------------------------------------------------------------------------------------------
N_INST, N_AGENTS, POLICY_STEPS = 2, 8, 16
_cache = {}


def _policy_case():
    if "case" not in _cache:
        from mapf_gpt_amd import maps
        from mapf_gpt_amd.model import build_model
        from mapf_gpt_amd.runner import make_instances
        grid, s_ok, g_ok = maps.load_named("validation-random-seed-000")
        pos, goal = make_instances(grid, 4, N_AGENTS, 0, s_ok, g_ok)             # instances 0..3: the shard test takes 2..3
        _cache["case"] = dict(grid=grid, pos=pos, goal=goal, net=build_model("tiny", seed=0, max_rows=4 * N_AGENTS, precision="f32"))
    return _cache["case"]


def _runner(lo=0, hi=N_INST, **kw):
    from mapf_gpt_amd.runner import BatchedRunner
    C = _policy_case()
    run = BatchedRunner(C["grid"], hi - lo, N_AGENTS, C["net"], max_episode_steps=POLICY_STEPS, seed=3, do_sample=True, precision="f32",
                        row_offset=lo * N_AGENTS, **kw)
    run.reset(C["pos"][lo:hi], C["goal"][lo:hi])
    return run


def _record(run, steps=POLICY_STEPS):
    """-> per step (actions, positions, done) as numpy, and the final overrides."""
    out = []
    for _ in range(steps):
        run.step()
        pos, _, done = run.env.sync_state()
        out.append((run.actions.cpu().numpy().copy(), pos.cpu().numpy().copy(), done.cpu().numpy().copy()))
    return out, run.shield_overrides().cpu().numpy() if run.shield else None


def _eager():
    if "eager" not in _cache:
        _cache["eager"] = _record(_runner(shield="pibt"))
    return _cache["eager"]


def test_through_the_policy_every_step_equals_the_restatement():
    C = _policy_case()
    run = _runner(shield="pibt")
    grids = np.asarray(C["grid"])[None]
    ref = sr.RefShield(grids, N_INST, N_AGENTS, POLICY_STEPS)
    ref.reset(C["pos"][:N_INST].numpy(), C["goal"][:N_INST].numpy())
    for t in range(POLICY_STEPS):
        before, skip = ref.pos.copy(), ref.done != 0
        run.step()
        logits, first, actions, planned = (x.cpu().numpy() for x in run.shield_state())
        live = ~skip
        want_act, want_planned = ref.step(sr.bits_of(logits).reshape(N_INST, N_AGENTS, 67), first)
        assert np.array_equal(actions[live], want_act[live]), f"actions differ at step {t}"
        assert np.array_equal(planned[live], want_planned[live]), f"planned cells differ at step {t}"
        pos, _, done = run.env.sync_state()
        assert np.array_equal(pos.cpu().numpy(), ref.pos) and np.array_equal(done.cpu().numpy(), ref.done)
        assert np.array_equal(pos.cpu().numpy()[live], planned[live]), "the env left an agent off its planned cell"
        ck.check_transition(grids, before, np.where(skip[:, None], 0, actions), np.where(skip[:, None, None], before, planned), ref.pos, skip)
        assert np.array_equal(run.shield_overrides().cpu().numpy(), ref.overrides)
    assert ref.overrides.sum() > 0                                        # the synthetic policy does run into conflicts


def test_graph_replay_equals_eager_and_two_runs_give_the_same_bits():
    want, want_over = _eager()
    for kw in ({"use_graph": True}, {}):
        got, over = _record(_runner(shield="pibt", **kw))
        for t, (a, b) in enumerate(zip(got, want)):
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (kw, t)
        assert np.array_equal(over, want_over)


def test_retire_mode_equals_the_plain_run_on_live_instances():
    want, want_over = _eager()
    run = _runner(shield="pibt", retire_done=True, poll_every=4)
    for t in range(POLICY_STEPS):
        live = (want[t - 1][2] if t else np.zeros(N_INST, np.uint8)) == 0
        run.step()
        pos, _, done = run.env.sync_state()
        assert np.array_equal(run.actions.cpu().numpy()[live], want[t][0][live]), t
        assert np.array_equal(pos.cpu().numpy(), want[t][1]) and np.array_equal(done.cpu().numpy(), want[t][2]), t
    assert np.array_equal(run.shield_overrides().cpu().numpy(), want_over)


def test_retire_mode_with_instances_that_retire():
    """64 instances x 2 agents with goals next to the starts (tests/test_gpu_retire.py's case b): instances finish all along the run, so
    the live list shrinks and stops being the identity while others run on.  The retire run equals the plain shielded run on the live
    instances, and the restatement applied to shield_state()'s compact logits through the live list gives the device's actions."""
    from mapf_gpt_amd.runner import BatchedRunner
    from tests.test_gpu_retire import _case
    from mapf_gpt_amd.model import build_model
    grid, pos, goal = _case("b")
    n_inst, n = pos.shape[:2]
    net = build_model("tiny", seed=0, max_rows=n_inst * n, precision="f32")
    mk = lambda **kw: BatchedRunner(grid, n_inst, n, net, max_episode_steps=128, seed=0, do_sample=True, precision="f32", shield="pibt", **kw)
    plain, ret = mk(), mk(retire_done=True, poll_every=4)
    plain.reset(pos, goal)
    ret.reset(pos, goal)
    ref = sr.RefShield(np.asarray(grid)[None], n_inst, n, 128)
    ref.reset(pos.numpy(), goal.numpy())
    counts, moved_ids = [], False
    for t in range(32):
        plain.step()
        ret.step()
        ids, logits = (x.cpu().numpy() for x in ret.live_state())
        counts.append(len(ids))
        moved_ids |= len(ids) > 0 and not np.array_equal(ids, np.arange(len(ids)))
        s_logits, first, actions, planned = (x.cpu().numpy() for x in ret.shield_state())
        assert np.array_equal(s_logits, logits)                           # retire mode: the compact rows of the live list
        running = np.array([i for i in ids if ref.done[i] == 0], np.int64)         # (an instance may finish inside the poll window)
        bits = np.zeros((n_inst, n, 67), np.uint32)
        bits[ids] = sr.bits_of(logits).reshape(len(ids), n, 67)
        want_act, want_planned = ref.step(bits, first, live=[int(i) for i in ids])
        assert np.array_equal(actions[running], want_act[running]), f"actions differ at step {t}"
        assert np.array_equal(planned[running], want_planned[running]), f"planned cells differ at step {t}"
        assert np.array_equal(actions[running], plain.actions.cpu().numpy()[running]), f"retire and plain differ at step {t}"
        for got, want in zip(ret.env.sync_state(), plain.env.sync_state()):
            assert np.array_equal(got.cpu().numpy(), want.cpu().numpy()), t
        assert np.array_equal(ret.env.sync_state()[0].cpu().numpy(), ref.pos) and np.array_equal(ret.env.sync_state()[2].cpu().numpy(), ref.done)
    assert counts[0] == n_inst and 0 < counts[-1] < n_inst and moved_ids, counts       # instances retired while others ran on
    assert np.array_equal(ret.shield_overrides().cpu().numpy(), plain.shield_overrides().cpu().numpy())
    assert np.array_equal(ret.shield_overrides().cpu().numpy(), ref.overrides)


def test_set_shield_is_refused_in_the_middle_of_a_replayed_episode():
    """The steps of a replayed graph never pass the host, so 'an episode is running' comes from the device: after the expert alone is
    reset and ONE replayed step has run, turning the shield off is MGPT_ERR_STATE; right after a reset it is allowed."""
    from mapf_gpt_amd import _lib
    L = _lib.lib()
    run = _runner(shield="pibt", use_graph=True)
    for _ in range(3):                                                    # eager, capture, replay
        run.step()
    run._shield.reset_shield()
    assert L.mgpt_step_set_shield(run._step, None) == _lib.OK             # (detached: the expert may be switched)
    assert L.mgpt_expert_set_shield(run._shield._h, 0) == _lib.OK         # nothing has run since its reset
    assert L.mgpt_expert_set_shield(run._shield._h, 1) == _lib.OK
    run._shield.reset_shield()
    assert L.mgpt_step_set_shield(run._step, run._shield._h) == _lib.OK
    for _ in range(3):                                                    # (the attach dropped the graph: capture again, then replay)
        run.step()
    run._shield.reset_shield()
    run.step()                                                            # a replayed step only
    assert L.mgpt_expert_set_shield(run._shield._h, 0) == _lib.ERR_STATE and b"middle of an episode" in L.mgpt_last_error()


def test_a_shard_equals_its_slice_of_the_unsharded_run():
    whole, whole_over = _record(_runner(0, 4, shield="pibt"), 8)
    shard, shard_over = _record(_runner(2, 4, shield="pibt"), 8)
    for t, (a, b) in enumerate(zip(whole, shard)):
        assert all(np.array_equal(x[2:], y) for x, y in zip(a, b)), t
    assert np.array_equal(whole_over[2:], shard_over)


def test_shield_none_is_the_runner_without_the_argument():
    from mapf_gpt_amd.runner import BatchedRunner
    C = _policy_case()
    outs = []
    for kw in ({"shield": None}, {}):
        run = BatchedRunner(C["grid"], N_INST, N_AGENTS, C["net"], max_episode_steps=POLICY_STEPS, seed=3, do_sample=True, precision="f32", **kw)
        run.reset(C["pos"][:N_INST], C["goal"][:N_INST])
        outs.append(_record(run, 8)[0])
        with pytest.raises(RuntimeError):
            run.shield_overrides()
    for a, b in zip(*outs):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    shielded = _eager()[0]
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(outs[0], shielded))     # and the shield does change the episode


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_the_stated_status():
    import torch
    from mapf_gpt_amd import _lib
    from mapf_gpt_amd.env import RULE_NO_FOLLOW, BatchedEnv
    from mapf_gpt_amd.expert import BatchedExpert
    from mapf_gpt_amd.observation_generator import BatchedTokenizer
    L = _lib.lib()
    case = CASES["agents8"]
    pos, goal = torch.from_numpy(case["pos"]), torch.from_numpy(case["goal"])
    mk = lambda **kw: BatchedExpert(case["grids"], 1, 8, 8, **kw)
    # together with search (and refine), swap, lifelong -- in either order
    for kw in ({"search": "lacam", "max_iters": 16}, {"search": "lacam", "max_iters": 16, "refine_rounds": 1}, {"swap": True}, {"lifelong": True}):
        ex = mk(**kw)
        assert L.mgpt_expert_set_shield(ex._h, 1) == _lib.ERR_UNSUPPORTED, kw
    ex = mk(shield=True)
    assert L.mgpt_expert_set_search(ex._h, 16, 0, 0) == _lib.ERR_UNSUPPORTED
    assert L.mgpt_expert_set_swap(ex._h, 1) == _lib.ERR_UNSUPPORTED
    assert L.mgpt_expert_set_lifelong(ex._h, 1) == _lib.ERR_UNSUPPORTED
    assert L.mgpt_expert_set_shield(ex._h, 2) == _lib.ERR_ARG
    # a non-zero env rule mask, a lifelong env
    ex = mk()
    ex.env.set_rules(RULE_NO_FOLLOW)
    assert L.mgpt_expert_set_shield(ex._h, 1) == _lib.ERR_UNSUPPORTED and b"rule" in L.mgpt_last_error()
    ex.env.set_rules(0)
    ex.env.set_lifelong(torch.from_numpy(np.broadcast_to(case["goal"][:, :, None, :], (1, 8, 4, 2)).copy()))
    assert L.mgpt_expert_set_shield(ex._h, 1) == _lib.ERR_UNSUPPORTED and b"lifelong" in L.mgpt_last_error()
    ex.env.set_lifelong(None)
    # call order: shield before set_shield / before reset; step and solve on a shield-mode context; in the middle of an episode
    logits = torch.zeros((8, 5), device="cuda")
    args = lambda e: (e._h, _lib.ptr(logits), 5, None, None, _lib.ptr(e.actions.view(-1)), _lib.stream_ptr())
    ex.reset(pos, goal)
    assert L.mgpt_expert_shield(*args(ex)) == _lib.ERR_STATE
    assert L.mgpt_expert_shield_commit(ex._h, _lib.stream_ptr()) == _lib.ERR_STATE
    assert L.mgpt_expert_copy_shield(ex._h, None, None, _lib.stream_ptr()) == _lib.ERR_STATE
    assert L.mgpt_expert_set_shield(ex._h, 1) == _lib.OK
    assert L.mgpt_expert_shield(*args(ex)) == _lib.ERR_STATE                     # a reset must follow set_shield
    ex.reset(pos, goal)
    assert L.mgpt_expert_shield(ex._h, _lib.ptr(logits), 4, None, None, _lib.ptr(ex.actions.view(-1)), _lib.stream_ptr()) == _lib.ERR_ARG
    assert L.mgpt_expert_shield(ex._h, _lib.ptr(logits), 5, _lib.ptr(ex.actions), None, _lib.ptr(ex.actions.view(-1)), _lib.stream_ptr()) == _lib.ERR_ARG
    assert L.mgpt_expert_step(ex._h, _lib.ptr(ex.actions.view(-1)), _lib.stream_ptr()) == _lib.ERR_STATE
    assert L.mgpt_expert_solve(ex._h, _lib.stream_ptr()) == _lib.ERR_STATE
    with pytest.raises(_lib.MGPTError):
        ex.step()
    ex.shield_step(logits, torch.zeros((1, 8), dtype=torch.int32))
    assert L.mgpt_expert_set_shield(ex._h, 0) == _lib.ERR_STATE and b"middle of an episode" in L.mgpt_last_error()
    # the step: an expert over other contexts, an expert that is not in shield mode, the logits read-back without a shield
    run = _runner()
    other = mk(shield=True)
    assert L.mgpt_step_set_shield(run._step, other._h) == _lib.ERR_ARG
    plain = BatchedExpert(None, N_INST, N_AGENTS, POLICY_STEPS, shield=True, env=run.env, tok=run.tok)
    assert L.mgpt_expert_set_shield(plain._h, 0) == _lib.OK
    assert L.mgpt_step_set_shield(run._step, plain._h) == _lib.ERR_STATE
    out = torch.empty((N_INST * N_AGENTS, 67), device="cuda")
    assert L.mgpt_step_copy_shield_logits(run._step, _lib.ptr(out), _lib.stream_ptr()) == _lib.ERR_STATE
    assert L.mgpt_step_set_shield(run._step, None) == _lib.OK
    with pytest.raises(ValueError):
        _runner(shield="lacam")
    with pytest.raises(NotImplementedError):
        _runner(shield="pibt").reset(_policy_case()["pos"][:N_INST], _policy_case()["goal"][:N_INST],
                                     goal_queue=torch.zeros((N_INST, N_AGENTS, 2, 2), dtype=torch.int16))


# ---- evaluation -------------------------------------------------------------------------------------------------------------------------
def test_evaluation_records_carry_shield_overrides_only_when_asked():
    from mapf_gpt_amd import evaluation as ev
    cfg = ev.load_yaml(os.path.join(ROOT, "eval_configs", "00-smoke", "00-smoke.yaml"))
    cfg["environment"]["seed"] = {"grid_search": [0]}
    cfg["environment"]["num_agents"] = {"grid_search": [8]}
    cfg["environment"]["max_episode_steps"] = 16
    cfg.pop("results_views", None)
    algo = dict(cfg["algorithms"]["MAPF-GPT-2M"], path_to_weights="synthetic:tiny", precision="f32")
    cfg["algorithms"] = {"plain": dict(algo), "shielded": dict(algo, shield="pibt")}
    res = ev.evaluation(cfg, print_fn=lambda *_: None)
    plain = [r for r in res if r["algorithm"] == "plain"]
    shielded = [r for r in res if r["algorithm"] == "shielded"]
    assert len(plain) == len(shielded) == 2
    assert all("shield_overrides" not in r["metrics"] for r in plain)
    for r in shielded:
        assert 0.0 <= r["metrics"]["shield_overrides"] <= 1.0
    assert any(r["metrics"]["shield_overrides"] > 0 for r in shielded)
    cfg["environment"]["on_target"] = "restart"
    cfg["algorithms"] = {"shielded": dict(algo, shield="pibt")}
    with pytest.raises(NotImplementedError):
        ev.evaluation(cfg, print_fn=lambda *_: None)


def test_the_list_api_ignores_the_field_with_one_warning():
    import warnings
    from mapf_gpt_amd.inference import MAPFGPTInference, MAPFGPTInferenceConfig
    algo = MAPFGPTInference(MAPFGPTInferenceConfig(path_to_weights="synthetic:tiny", precision="f32", shield="pibt"))
    rows = [[0] * 256, [1] * 256]                                        # pre-tokenised observations of two agents
    with pytest.warns(UserWarning, match="shield"):
        first = algo.act(rows)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        again = algo.act(rows)
    assert not [w for w in seen if "shield" in str(w.message)]
    assert len(first) == len(again) == 2 and all(0 <= a <= 4 for a in first + again)
