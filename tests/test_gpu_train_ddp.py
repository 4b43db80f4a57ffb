"""Data-parallel training on the device (GPT.grads_size / export_grads / reduce_grads; python -m mapf_gpt_amd.training under RANK /
WORLD_SIZE): the flat gradient buffer and the rank-ordered sum are exact, two ranks sharing the one GPU over gloo train bit for bit as one
process that replays them with the public pieces, the RCCL branch with one rank equals the plain run, and bf16 rides along."""
import ctypes
import json
import math
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from mapf_gpt_amd import _lib, training, weights
from mapf_gpt_amd.model import GPT, GPTConfig, build_model
from tests.helpers import GOLDEN, ROOT
from tests.train_ref import loss_and_grads, targets_last

pytestmark = pytest.mark.gpu


def _fixture_rows(name, n):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    return d["inputs"][:n].astype(np.int8), d["gt_actions"][:n].astype(np.int8)


def _tiny(max_rows=4, seed=0):
    return build_model("tiny", seed=seed, max_rows=max_rows).train()


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _one_step(net, rows=3):
    x, y = _fixture_rows("ds_random", rows)
    net.zero_grad()
    net.forward_backward(torch.as_tensor(x), torch.as_tensor(targets_last(y)))


def test_export_and_reduce_are_exact():
    net = _tiny()
    _one_step(net)
    n = net.grads_size()
    assert n >= sum(math.prod(shp) for _, shp in net.named_parameters())
    flat = net.export_grads()
    assert flat.shape == (n,) and flat.dtype == torch.float32 and flat.is_cuda
    named = net.grads()
    # exactly rounded sums (math.fsum) do not depend on the order: equal sums of squares = nothing but zeros outside the named tensors
    sq_flat = math.fsum((flat.double().cpu().numpy() ** 2).tolist())
    sq_named = math.fsum(np.concatenate([(g.double().cpu().numpy() ** 2).ravel() for g in named.values()]).tolist())
    assert sq_flat == sq_named and sq_flat > 0
    into = torch.full((n,), 7.0, device="cuda")
    assert net.export_grads(into) is into and torch.equal(into, flat)
    with pytest.raises(ValueError):
        net.export_grads(torch.empty(n - 1, device="cuda"))
    # one buffer times 1.0 is the buffer; times 0.5 every element is exactly half
    net.reduce_grads(flat[None], 1.0)
    for k, g in net.grads().items():
        assert np.array_equal(_bits(g), _bits(named[k])), k
    net.reduce_grads(flat[None], 0.5)
    assert np.array_equal(_bits(net.export_grads()), (np.float32(0.5) * flat.cpu().numpy()).view(np.int32))
    half = net.export_grads().clone()
    # refusals: MGPT_ERR_ARG for a NULL pointer, a wrong n_elem, world < 1 and a scale that is not finite and positive
    L, h, s = _lib.lib(), net._h, _lib.stream_ptr()
    assert L.mgpt_gpt_grads_size(h, None) == _lib.ERR_ARG
    assert L.mgpt_gpt_grads_export(h, None, n, s) == _lib.ERR_ARG
    for bad in (n - 1, n + 1, 0):
        assert L.mgpt_gpt_grads_export(h, _lib.ptr(into), bad, s) == _lib.ERR_ARG, bad
    assert L.mgpt_gpt_grads_reduce(h, None, 1, 1.0, s) == _lib.ERR_ARG
    for world in (0, -1):
        assert L.mgpt_gpt_grads_reduce(h, _lib.ptr(flat), world, 1.0, s) == _lib.ERR_ARG, world
    for scale in (0.0, -0.5, float("inf"), float("nan")):
        with pytest.raises(_lib.MGPTError) as e:
            net.reduce_grads(flat[None], scale)
        assert e.value.code == _lib.ERR_ARG, scale
    with pytest.raises(ValueError):
        net.reduce_grads(flat[: n - 1], 1.0)
    with pytest.raises(ValueError):
        net.reduce_grads(flat.double()[None], 1.0)
    torch.cuda.synchronize()
    assert torch.equal(into, flat) and np.array_equal(_bits(net.export_grads()), _bits(half))      # a refused call touches nothing
    # ... and MGPT_ERR_STATE without a training workspace
    cold = build_model("tiny", seed=0, max_rows=4)
    cnt = ctypes.c_int64(0)
    assert L.mgpt_gpt_grads_size(cold._h, ctypes.byref(cnt)) == _lib.ERR_STATE
    assert L.mgpt_gpt_grads_export(cold._h, _lib.ptr(into), n, s) == _lib.ERR_STATE
    assert L.mgpt_gpt_grads_reduce(cold._h, _lib.ptr(flat), 1, 1.0, s) == _lib.ERR_STATE
    for call in (cold.grads_size, cold.export_grads, lambda: cold.reduce_grads(flat[None], 1.0)):
        with pytest.raises(RuntimeError, match="train"):
            call()


def _spread(world, n, seed):
    """float32 [world][n], magnitudes 2^-20 .. 2^20 with mixed signs: sums whose value depends on the order of the additions"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return (np.where(rng.random((world, n)) < 0.5, -1.0, 1.0) * np.exp2(rng.uniform(-20, 20, (world, n)))).astype(np.float32)


def _in_rank_order(g, scale):
    s = g[0].copy()
    for r in range(1, len(g)):
        s = s + g[r]                                   # float32 + float32, one rank after the other
    assert s.dtype == np.float32
    return np.float32(scale) * s


def test_reduce_adds_in_rank_order():
    net = _tiny()
    n = net.grads_size()
    g = _spread(3, n, 5)
    a, b, c = g
    differ = ((a + b) + c != a + (b + c)).mean()       # a condition on the input: an order-blind sum cannot match all of these
    assert differ >= 0.10, differ
    want = _in_rank_order(g, 1.0 / 3.0)
    net.reduce_grads(torch.as_tensor(g).cuda(), 1.0 / 3.0)
    assert np.array_equal(_bits(net.export_grads()), want.view(np.int32))
    assert not np.array_equal(want, np.float32(1.0 / 3.0) * (a + (b + c)))
    # the same array 4 bytes off a 16-byte boundary: no wide access is possible and the element-by-element loop takes all of it, the last
    # n % 4 elements included (n % 4 == 0 for every model this library creates, so this is how that loop is reached)
    store = torch.zeros(3 * n + 1, device="cuda")
    off = store[1:].view(3, n)
    off.copy_(torch.as_tensor(g))
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    net.zero_grad()
    net.reduce_grads(off, 1.0 / 3.0)
    assert np.array_equal(_bits(net.export_grads()), want.view(np.int32))
    for world in (1, 8):
        g = _spread(world, n, 6 + world)
        for src in (torch.as_tensor(g).cuda(), None):
            if src is None:
                store = torch.zeros(world * n + 1, device="cuda")
                src = store[1:].view(world, n)
                src.copy_(torch.as_tensor(g))
            net.zero_grad()
            net.reduce_grads(src, 1.0 / world)
            assert np.array_equal(_bits(net.export_grads()), _in_rank_order(g, 1.0 / world).view(np.int32)), world


# ----- the command under RANK / WORLD_SIZE -----
BATCH, ACCUM, SEED = 8, 4, 1337
SCHEDULE = dict(learning_rate=1e-3, warmup_iters=2, lr_decay_iters=6, min_lr=1e-4)
EVAL_INTERVAL, EVAL_ITERS = 2, 2


def _write_shard(pa, path, x, y):
    table = pa.table({"input_tensors": pa.array(list(x)), "gt_actions": pa.array(y)})
    with pa.OSFile(str(path), "wb") as sink:
        with pa.ipc.new_file(sink, table.schema) as w:
            w.write_table(table)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """a training directory of 4 shard files (48 rows each) and a validation shard, from the committed dataset fixtures"""
    pa = pytest.importorskip("pyarrow")
    root = tmp_path_factory.mktemp("ddp")
    train = root / "train"
    train.mkdir()
    for k, name in enumerate(("ds_random", "ds_maze", "ds_maskc2g", "ds_lifelong")):
        _write_shard(pa, train / f"part_{k}.arrow", *_fixture_rows(name, 48))
    _write_shard(pa, root / "val.arrow", *_fixture_rows("ds_short", 20))
    return root


def _command(data, out_dir, *extra):
    return [sys.executable, "-m", "mapf_gpt_amd.training", "--init", "tiny", "--data", str(data / "train"), "--val", str(data / "val.arrow"),
            "--out-dir", str(out_dir), "--gradient-accumulation-steps", str(ACCUM), "--batch-size", str(BATCH),
            "--eval-interval", str(EVAL_INTERVAL), "--eval-iters", str(EVAL_ITERS), "--warmup-iters", str(SCHEDULE["warmup_iters"]),
            "--lr-decay-iters", str(SCHEDULE["lr_decay_iters"]), "--learning-rate", str(SCHEDULE["learning_rate"]),
            "--min-lr", str(SCHEDULE["min_lr"]), *extra]


def _plain_env(**more):
    env = dict(os.environ, **more)
    if "RANK" not in more:
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE"):
            env.pop(k, None)
    return env


def _run_all(jobs, timeout):
    """jobs [(cmd, env)] as fresh child processes side by side under ONE time limit: on expiry every child is killed and the test fails"""
    procs = [subprocess.Popen(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for cmd, env in jobs]
    deadline = time.monotonic() + timeout
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=max(0.1, deadline - time.monotonic())))
    except subprocess.TimeoutExpired:
        for p in procs:
            p.kill()
        tails = [p.communicate()[1][-1500:] for p in procs]
        pytest.fail(f"the child processes did not finish within {timeout} s; stderr tails: {tails}")
    for p, (_, err) in zip(procs, outs):
        assert p.returncode == 0, err[-3000:]
    return [[json.loads(l) for l in out.splitlines() if l.startswith("{")] for out, _ in outs], [out for out, _ in outs]


def _two_ranks(data, tmp_path, port, *extra):
    jobs = []
    for r in (0, 1):
        env = _plain_env(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        jobs.append((_command(data, tmp_path / f"out{r}", "--backend", "gloo", "--share-gpu", *extra), env))
    lines, raw = _run_all(jobs, 600)
    # the master alone prints its JSON lines and writes (gloo itself may report its connections on any rank's stdout)
    assert lines[1] == [] and not (tmp_path / "out1").exists(), raw[1][-500:]
    final = lines[0][-1]
    assert final["world"] == 2 and len(final["param_checksums"]) == 2 and final["param_checksums"][0] == final["param_checksums"][1]
    return lines[0], tmp_path / "out0" / "ckpt.pt"


def _replay(data, max_iters, precision):
    """The two ranks' run in one process, from the public pieces: per iteration each rank's micro-steps from its own iterator into
    gathered[r], the rank-ordered mean, clip, AdamW.  The master's estimate_loss draws eval_iters training batches at every eval_interval
    boundary (train.py:250-251) after the loop's first batch was fetched; they are drawn here too.
    -> (net, state_dict after the last checkpointed iteration, first iteration's micro-batches and mean gradients)"""
    sd = weights.synthetic_state_dict("tiny", seed=SEED)
    net = GPT(GPTConfig(**weights.model_args("tiny")), max_rows=BATCH, precision="f32")
    net.load_state_dict(sd)
    net.train(max_rows=BATCH)
    opt = net.configure_optimizers(training.DEFAULTS["weight_decay"], SCHEDULE["learning_rate"],
                                   (training.DEFAULTS["beta1"], training.DEFAULTS["beta2"]))
    its = [iter(training.ArrowBatches(str(data / "train"), BATCH, SEED, r, 2)) for r in (0, 1)]
    cur = [next(it) for it in its]
    gathered = torch.empty((2, net.grads_size()), dtype=torch.float32, device="cuda")
    per_rank = ACCUM // 2
    saved, first = None, None
    for iter_num in range(max_iters + 1):
        lr = training.get_lr(iter_num, **SCHEDULE)
        for g in opt.param_groups:
            g["lr"] = lr
        if iter_num % EVAL_INTERVAL == 0:
            if iter_num > 0:
                saved = {k: v.cpu() for k, v in net.state_dict().items()}
            for _ in range(EVAL_ITERS):
                next(its[0])
        micro = []
        for r in (0, 1):
            net.zero_grad()
            for _ in range(per_rank):
                micro.append(cur[r])
                net.forward_backward(torch.as_tensor(cur[r][0]), torch.as_tensor(cur[r][1]), loss_scale=1.0 / per_rank, precision=precision)
                cur[r] = next(its[r])
            net.export_grads(gathered[r])
        net.reduce_grads(gathered, 0.5)
        if first is None:
            first = (micro, {k: v.double().cpu() for k, v in net.grads().items()})
        net.clip_grad_norm_(training.DEFAULTS["grad_clip"])
        opt.step()
        opt.zero_grad(set_to_none=True)
    return net, saved, first


def test_two_ranks_equal_one_process(data, tmp_path):
    lines, ckpt = _two_ranks(data, tmp_path, 29561, "--max-iters", "3")
    evals = [l for l in lines if "val_loss" in l]
    assert [e["iter"] for e in evals] == [0, 2] and lines[-1]["iter"] == 4
    net, saved, (micro, g_first) = _replay(data, 3, "f32")
    assert training.param_checksum(net) == lines[-1]["param_checksums"][0]
    raw = torch.load(ckpt, map_location="cpu", weights_only=True)
    assert raw["iter_num"] == 2 and raw["config"]["gradient_accumulation_steps"] == ACCUM
    assert set(raw["model"]) == set(saved)
    for k, v in raw["model"].items():
        assert np.array_equal(_bits(v), _bits(saved[k])), k
    # the first iteration's synchronised gradients against fp64 autograd of the four micro-batches at 1 / 4 each: the accumulation bar of
    # tests/test_gpu_train.py, unchanged
    from tests.test_gpu_train import _check_grads
    assert len(micro) == ACCUM
    sd, args = weights.synthetic_state_dict("tiny", seed=SEED), weights.model_args("tiny")
    _, g64 = loss_and_grads(sd, args, None, None, torch.float64, 1.0 / ACCUM, micro=micro)
    _, g32 = loss_and_grads(sd, args, None, None, torch.float32, 1.0 / ACCUM, micro=micro)
    assert set(g_first) == set(g64)
    _check_grads("two ranks", g_first, g64, g32)


def test_rccl_branch_with_one_rank_equals_the_plain_run(data, tmp_path):
    one = _plain_env(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29567", HSA_ENABLE_IPC_MODE_LEGACY="0")
    jobs = [(_command(data, tmp_path / "rccl", "--backend", "nccl", "--max-iters", "3"), one),
            (_command(data, tmp_path / "plain", "--max-iters", "3"), _plain_env())]
    (rccl, plain), _ = _run_all(jobs, 600)
    assert rccl[-1]["world"] == 1 and len(rccl[-1]["param_checksums"]) == 1
    assert "world" not in plain[-1] and "param_checksums" not in plain[-1]
    def unsaved(ls):
        return [{k: v for k, v in l.items() if k != "saved"} for l in ls]
    assert unsaved(rccl[:-1]) == unsaved(plain[:-1]) and len(plain) == 3          # the evaluations at 0 and 2 print the same losses
    assert {k: v for k, v in rccl[-1].items() if k not in ("world", "param_checksums")} == plain[-1]
    a = torch.load(tmp_path / "rccl" / "ckpt.pt", map_location="cpu", weights_only=True)
    b = torch.load(tmp_path / "plain" / "ckpt.pt", map_location="cpu", weights_only=True)
    assert a["iter_num"] == b["iter_num"] == 2 and set(a["model"]) == set(b["model"])
    for k in a["model"]:
        assert np.array_equal(_bits(a["model"][k]), _bits(b["model"][k])), k
    sa, sb = a["optimizer"]["state"], b["optimizer"]["state"]
    assert set(sa) == set(sb) and len(sa) > 0 and a["optimizer"]["param_groups"] == b["optimizer"]["param_groups"]
    for i in sa:
        assert float(sa[i]["step"]) == float(sb[i]["step"]) == 2.0
        for k in ("exp_avg", "exp_avg_sq"):
            assert np.array_equal(_bits(sa[i][k]), _bits(sb[i][k])), (i, k)


def test_bf16_two_ranks_equal_one_process(data, tmp_path):
    lines, _ = _two_ranks(data, tmp_path, 29573, "--dtype", "bfloat16", "--max-iters", "2")
    net, _, _ = _replay(data, 2, "bf16")
    assert training.param_checksum(net) == lines[-1]["param_checksums"][0]
