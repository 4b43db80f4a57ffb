"""Retire mode on the device: the ordered live list, the sampler on compact logits, and BatchedRunner(retire_done=True) against the
plain runner -- bit for bit in fp32, by a host replay of its own actions where the 16-bit call regime changes with the row count."""
import ctypes

import numpy as np
import pytest
import torch

from mapf_gpt_amd import _lib, maps

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 1024, 1025, 4097]       # wave, workgroup-pass and multi-pass boundaries of live_list_kernel
MAP = "puzzle-00"


def _patterns(n):
    rng = np.random.Generator(np.random.PCG64([n, 5]))
    first, last, alt = np.ones(n, np.uint8), np.ones(n, np.uint8), np.ones(n, np.uint8)
    first[0], last[-1], alt[::2] = 0, 0, 0
    return {"all live": np.zeros(n, np.uint8), "none live": np.full(n, 2, np.uint8), "only the first": first, "only the last": last,
            "alternating": alt, "random 0/1/2": rng.integers(0, 3, n).astype(np.uint8)}


def _live_list(done_np):
    """mgpt_live_list on the device -> (live int32 [n] device tensor, count device tensor)."""
    n = len(done_np)
    done = torch.from_numpy(done_np).cuda()
    live = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().mgpt_live_list(_lib.ptr(done), n, _lib.ptr(live), _lib.ptr(count), _lib.stream_ptr()))
    return live, count


# ---- 1. the live list --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_inst", SIZES)
def test_live_list_equals_flatnonzero(n_inst):
    for name, done in _patterns(n_inst).items():
        want = np.flatnonzero(done == 0).astype(np.int32)
        live, count = _live_list(done)
        again, count2 = _live_list(done)
        got, k = live.cpu().numpy(), int(count.cpu()[0])
        assert k == len(want), (name, k, len(want))
        assert np.array_equal(got[:k], want), name
        assert (got[k:] == -1).all(), name                                      # the tail is defined too
        assert torch.equal(live, again) and torch.equal(count, count2), name    # same flags, same bits


# ---- 2. the live sampler -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("do_sample", [0, 1])
@pytest.mark.parametrize("n_agents", [1, 2, 13])
def test_live_sampler_writes_what_the_full_sampler_writes(n_agents, do_sample):
    L = _lib.lib()
    gen = torch.Generator().manual_seed(n_agents)
    for n_inst in (65, 257):
        R = n_inst * n_agents
        logits = (torch.randn((R, 67), generator=gen) * 2.0).cuda()
        for name, done in _patterns(n_inst).items():
            live, count = _live_list(done)
            ids = np.flatnonzero(done == 0)
            compact = logits.view(n_inst, n_agents, 67)[torch.from_numpy(ids).cuda()].reshape(-1, 67).contiguous()
            if len(ids) == 0:
                compact = torch.zeros((1, 67), device="cuda")                   # (never read: the count is 0)
            for row0 in (0, 3 * R + 5):
                full = torch.empty((R,), dtype=torch.int32, device="cuda")
                _lib.check(L.mgpt_sample_actions(_lib.ptr(logits), R, _lib.ptr(full), do_sample, 11, 3, row0, _lib.stream_ptr()))
                got = torch.full((R,), -9, dtype=torch.int32, device="cuda")
                _lib.check(L.mgpt_sample_actions_live(_lib.ptr(compact), _lib.ptr(live), _lib.ptr(count), n_agents, _lib.ptr(got), do_sample,
                                                      11, 3, row0, _lib.stream_ptr()))
                is_live = np.repeat(done == 0, n_agents)
                full, got = full.cpu().numpy(), got.cpu().numpy()
                assert np.array_equal(got[is_live], full[is_live]), (name, n_inst, row0)
                assert (got[~is_live] == -9).all(), (name, n_inst, row0)        # rows of retired instances keep the sentinel
            if do_sample and len(ids) > 8:
                assert len(np.unique(full)) > 1                                 # (a real draw, not a constant)


# ---- 3. the runner in fp32 equals the plain runner bit for bit ---------------------------------------------------------------------
def _near_goals(grid, pos, i):
    """Goals next to the starts, so that two-agent episodes finish: for agent a in order, a seeded choice among the free cells within
    Manhattan distance 1 of its start (the start itself included) that no earlier agent of the instance took."""
    free = np.argwhere(grid == 0)
    rng = np.random.Generator(np.random.PCG64([i, 77]))
    goal, taken = np.array(pos).copy(), set()
    for a in range(len(pos)):
        d = np.abs(free - pos[a]).sum(1)
        cand = [tuple(c) for c in free[d <= 1] if tuple(c) not in taken]
        c = cand[rng.integers(0, len(cand))]
        taken.add(c)
        goal[a] = c
    return goal


def _case(which):
    grid, s_ok, g_ok = maps.load_named(MAP)
    n_inst, n = (48, 1) if which == "a" else (64, 2)
    pos = np.empty((n_inst, n, 2), np.int16)
    goal = np.empty((n_inst, n, 2), np.int16)
    for i in range(n_inst):
        pos[i], goal[i] = maps.place_agents(grid, n, i, s_ok, g_ok)
        if which == "b":
            goal[i] = _near_goals(grid, pos[i], i)
    return grid, torch.from_numpy(pos), torch.from_numpy(goal)


_plain_cache = {}


def _plain_run(which, steps=64):
    """The plain runner's episode, computed once per case: actions after every step, done flags after 0 .. steps steps, final state, metrics."""
    if which not in _plain_cache:
        from mapf_gpt_amd.model import build_model
        from mapf_gpt_amd.runner import BatchedRunner
        grid, pos, goal = _case(which)
        n_inst, n = pos.shape[:2]
        net = build_model("tiny", seed=0, max_rows=n_inst * n, precision="f32")
        run = BatchedRunner(grid, n_inst, n, net, max_episode_steps=128, seed=0, do_sample=True, precision="f32")
        run.reset(pos, goal)
        acts, done = [], [np.zeros(n_inst, np.uint8)]
        for _ in range(steps):
            run.step()
            acts.append(run.actions.clone())
            done.append(run.env.sync_state()[2].cpu().numpy().copy())
        state = [x.clone() for x in run.env.sync_state()]
        _plain_cache[which] = {"net": net, "grid": grid, "pos": pos, "goal": goal, "acts": acts, "done": done, "state": state,
                               "metrics": run.metrics().clone()}
    return _plain_cache[which]


@pytest.mark.parametrize("poll_every", [1, 8])
@pytest.mark.parametrize("which", ["a", "b"])
def test_fp32_retire_run_equals_the_plain_run(which, poll_every):
    from mapf_gpt_amd.runner import BatchedRunner
    steps = 64
    P = _plain_run(which, steps)
    n_inst, n = P["pos"].shape[:2]
    done = P["done"]
    # preconditions on the plain run: instances do retire, and a good part of the batch is still live at the last poll
    assert np.count_nonzero(done[steps // 2]) >= n_inst // 4, np.count_nonzero(done[steps // 2])
    last_poll = ((steps - 1) // poll_every) * poll_every
    assert np.count_nonzero(done[last_poll] == 0) >= n_inst // 4, np.count_nonzero(done[last_poll] == 0)
    run = BatchedRunner(P["grid"], n_inst, n, P["net"], max_episode_steps=128, seed=0, do_sample=True, precision="f32",
                        retire_done=True, poll_every=poll_every)
    run.reset(P["pos"], P["goal"])
    assert run.live_instances == n_inst and run.rows_forwarded == 0
    want_rows = 0
    for t in range(steps):
        run.step()
        live = done[(t // poll_every) * poll_every] == 0                       # the governing poll saw the flags after that many steps
        assert run.live_instances == np.count_nonzero(live), t
        want_rows += np.count_nonzero(live) * n
        idx = torch.from_numpy(np.flatnonzero(live)).cuda()
        assert torch.equal(run.actions[idx], P["acts"][t][idx]), f"actions of the live instances, step {t}"
    assert run.t == steps and run.rows_forwarded == want_rows and want_rows < steps * n_inst * n
    for got, want in zip(run.env.sync_state(), P["state"]):
        assert torch.equal(got, want)
    assert torch.equal(run.metrics(), P["metrics"])


def test_run_returns_early_when_nothing_is_live():
    from mapf_gpt_amd.runner import BatchedRunner
    P = _plain_run("a")
    n_inst, n = P["pos"].shape[:2]
    runs = [BatchedRunner(P["grid"], n_inst, n, P["net"], max_episode_steps=12, seed=0, do_sample=True, precision="f32", **kw)
            for kw in ({}, {"retire_done": True, "poll_every": 8})]
    for r in runs:                                  # every instance is truncated at step 12: the poll before step 16 finds none live
        r.reset(P["pos"], P["goal"])
        r.run(64)
    plain, ret = runs
    assert plain.t == 64 and ret.t == 16 and ret.live_instances == 0
    assert ret.rows_forwarded == (n_inst + np.count_nonzero(P["done"][8] == 0)) * 8 * n
    assert torch.equal(ret.metrics(), plain.metrics())
    for got, want in zip(ret.env.sync_state(), plain.env.sync_state()):
        assert torch.equal(got, want)
    ret.reset(P["pos"], P["goal"])                  # reset makes every instance live again
    assert ret.live_instances == n_inst and ret.rows_forwarded == 0 and ret.t == 0
    ret.step()
    assert torch.equal(ret.actions, P["acts"][0])


# ---- 4. f16x3 across the 128-row boundary ------------------------------------------------------------------------------------------
def test_f16x3_retire_run_crosses_the_small_call_boundary():
    """6M, 144 instances x 1 agent: the policy call starts above kSmallRows (128) and drops below it at the poll before step 4 (the
    CPU oracle gives live counts 144, 127, 121, 118, 118, 116).  The two regimes run different kernels, so the retire run need not equal
    the plain run bit for bit; it must be a correct episode of its own: a host replay of every instance from the run's recorded actions
    gives the device's metrics, and the compact call's logits are the policy's logits of those rows."""
    from mapf_gpt_amd.model import build_model
    from mapf_gpt_amd.runner import BatchedRunner
    from tests.test_gpu_evaluation import _replay_metrics
    grid, s_ok, g_ok = maps.load_named(MAP)
    n_inst, steps, poll_every = 144, 24, 4
    pos = np.empty((n_inst, 1, 2), np.int16)
    goal = np.empty((n_inst, 1, 2), np.int16)
    for i in range(n_inst):
        pos[i], goal[i] = maps.place_agents(grid, 1, i, s_ok, g_ok)
    net = build_model("6M", seed=0, max_rows=n_inst, precision="f16x3")
    run = BatchedRunner(grid, n_inst, 1, net, max_episode_steps=steps, seed=0, do_sample=True, precision="f16x3", retire_done=True,
                        poll_every=poll_every)
    run.reset(torch.from_numpy(pos), torch.from_numpy(goal))
    acts, counts, err, bar = [], [], None, None
    for t in range(steps):
        run.step()
        if t % poll_every == 0:
            counts.append(run.live_instances)
        if t == 4:
            ids, logits = run.live_state()
            assert len(ids) == run.live_instances and logits.shape == (run.live_instances, 67)
            want = net.logits_tokens(run.tokens[ids.long()].contiguous())
            err, bar = float((logits - want).abs().max()), net.envelope()["probe_tol"]
        acts.append(run.actions.cpu().numpy().copy())
    print("live counts at the polls:", counts, " compact logits vs plain call:", err, "bar", bar)
    assert counts[0] > 128 and min(counts[1:]) <= 128, counts
    assert net.envelope()["effective_precision"] == "f16x3"
    assert err <= bar, (err, bar)
    m = run.metrics().cpu().numpy()
    for i in range(n_inst):
        want = _replay_metrics(grid, pos[i], goal[i], [a[i] for a in acts], steps)
        for j, key in enumerate(("CSR", "ISR", "SoC", "makespan", "ep_length")):
            assert m[i, j] == pytest.approx(want[key], rel=0, abs=1e-6), (i, key, m[i, j], want[key])
    assert (m[:, 0] == 1.0).sum() >= 16                # (episodes did finish: the retired rows were really skipped)


# ---- 5. harness, refusals, switching back ------------------------------------------------------------------------------------------
def test_evaluation_records_do_not_change():
    from mapf_gpt_amd import evaluation as ev
    cfg = {"environment": {"name": "Environment", "on_target": "nothing", "max_episode_steps": 256,
                           "seed": {"grid_search": list(range(12))}, "num_agents": {"grid_search": [1, 2]}, "map_name": MAP},
           "algorithms": {"A": {"name": "MAPF-GPT", "path_to_weights": "synthetic:tiny", "precision": "f32"}}}
    strip = lambda res: [{**r, "metrics": {k: v for k, v in r["metrics"].items() if k != "runtime"}} for r in res]
    plain = strip(ev.evaluation(cfg, print_fn=lambda *_: None, retire_done=False))
    ret = strip(ev.evaluation(cfg, print_fn=lambda *_: None, retire_done=True))
    assert len(plain) == 24 and ret == plain
    assert any(r["metrics"]["CSR"] == 1.0 for r in plain)


def test_graph_replay_is_refused_and_retire_can_be_switched_off():
    from mapf_gpt_amd.runner import BatchedRunner
    P = _plain_run("a")
    n_inst, n = P["pos"].shape[:2]
    mk = lambda **kw: BatchedRunner(P["grid"], n_inst, n, P["net"], max_episode_steps=128, seed=0, do_sample=True, precision="f32", **kw)
    with pytest.raises(ValueError):
        mk(use_graph=True, retire_done=True)
    run = mk(retire_done=True, poll_every=1)
    run.reset(P["pos"], P["goal"])
    rc = _lib.lib().mgpt_step_run(run._step, _lib.ptr(run.tokens), _lib.ptr(run.actions.view(-1)), 0, 1, _lib.stream_ptr())
    assert rc == _lib.ERR_UNSUPPORTED                  # the C ABI refuses as well, before anything is launched
    run.run(16)
    assert run.live_instances < n_inst
    # mgpt_step_set_retire(step, 0): a plain step again -- EVERY row is forwarded and sampled, the retired instances' too
    run.set_retire_done(False)
    n_live = ctypes.c_int(0)
    assert _lib.lib().mgpt_step_poll_live(run._step, ctypes.byref(n_live), _lib.stream_ptr()) == _lib.ERR_STATE
    run.reset(P["pos"], P["goal"])
    for t in range(16):
        run.step()
        assert torch.equal(run.actions, P["acts"][t]), t
    assert run.rows_forwarded == 16 * n_inst * n
