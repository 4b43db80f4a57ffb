"""CPU checks of data-parallel training (mapf_gpt_amd/training.py under a launcher's RANK / WORLD_SIZE; train.py:118-138): the binding of
mgpt_gpt_grads_size / _export / _reduce, the deal of the training split's files to the ranks (fast_data_loader.py:20-28) with the shuffle seed
seed + rank, the division of gradient_accumulation_steps, the new flags, and that rank_reduce_kernel compiles for gfx950 without scratch."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from mapf_gpt_amd import _lib, training
from tests.helpers import ROOT

REQUIRED = ["--init", "tiny", "--data", "a.arrow", "--val", "b.arrow"]


def test_grads_symbols_are_bound_and_check_their_arguments_without_gpu():
    from mapf_gpt_amd import build
    build.build()
    L = _lib.lib()
    for name in ("mgpt_gpt_grads_size", "mgpt_gpt_grads_export", "mgpt_gpt_grads_reduce"):
        assert name in _lib.SYMBOLS and _lib.SYMBOLS[name][0] is ctypes.c_int, name
    assert _lib.SYMBOLS["mgpt_gpt_grads_reduce"][1][3] is ctypes.c_float
    n = ctypes.c_int64(-1)
    calls = [lambda: L.mgpt_gpt_grads_size(None, ctypes.byref(n)),
             lambda: L.mgpt_gpt_grads_export(None, None, 0, None),
             lambda: L.mgpt_gpt_grads_reduce(None, None, 2, 0.5, None)]
    for call in calls:
        L.mgpt_gpt_create(ctypes.byref(ctypes.c_void_p()), 2, 3, 64, 256, 4)       # leaves another message (n_embd % n_head) behind
        assert b"NULL" not in L.mgpt_last_error()
        assert call() == _lib.ERR_ARG
        assert b"NULL" in L.mgpt_last_error()
    assert n.value == -1


def _write_shard(pa, path, x, y):
    table = pa.table({"input_tensors": pa.array(list(x)), "gt_actions": pa.array(y)})
    with pa.OSFile(str(path), "wb") as sink:
        with pa.ipc.new_file(sink, table.schema) as w:
            w.write_table(table)


def _restated(shards, seed, rounds, batch):
    """tests/test_train_cpu.py::test_batches_match_fast_data_loader's restatement over `shards`: files in order, forever; each file shuffled
    when it is loaded (one generator), targets -1 but position 255"""
    g = np.random.Generator(np.random.PCG64(seed))
    want = []
    for _ in range(rounds):
        for x, y in shards:
            idx = g.permutation(len(x))
            xs, ys = x[idx], y[idx]
            t = np.full(xs.shape, -1, np.int64)
            t[:, -1] = ys
            want += [(xs[i:i + batch], t[i:i + batch]) for i in range(0, len(xs), batch)]
    return want


def test_files_are_dealt_to_the_ranks_with_seed_plus_rank(tmp_path):
    pa = pytest.importorskip("pyarrow")
    rng = np.random.Generator(np.random.PCG64(11))
    shards = []
    for k, n in enumerate((5, 3, 4, 6, 2)):
        x = rng.integers(0, 67, (n, 256)).astype(np.int8)
        y = rng.integers(0, 5, n).astype(np.int8)
        _write_shard(pa, tmp_path / f"part_{k}.arrow", x, y)
        shards.append((x, y))
    names = [str(tmp_path / f"part_{k}.arrow") for k in range(5)]
    seed = 7
    for rank, mine in ((0, [0, 1]), (1, [2, 3])):                   # 5 // 2 = 2 files each; file 4 is never read
        b = training.ArrowBatches(str(tmp_path), 2, seed, rank, 2)
        assert b.files == [names[k] for k in mine]
        it = iter(b)
        for wx, wt in _restated([shards[k] for k in mine], seed + rank, 3, 2):
            gx, gt = next(it)
            assert np.array_equal(gx, wx) and np.array_equal(gt, wt)
    assert training.rank_files(names, 2, 5) == [names[2]] and training.rank_files(names, 0, 1) == names
    # rank 0 of a world of 1 is today's iterator, batch for batch (positional signature and keywords)
    old, new = iter(training.ArrowBatches(str(tmp_path), 2, seed=seed)), iter(training.ArrowBatches(str(tmp_path), 2, seed, rank=0, world=1))
    for wx, wt in _restated(shards, seed, 2, 2):
        for it in (old, new):
            gx, gt = next(it)
            assert np.array_equal(gx, wx) and np.array_equal(gt, wt)
    with pytest.raises(ValueError, match=r"6 ranks.*5 "):
        training.ArrowBatches(str(tmp_path), 2, seed, 0, 6)
    with pytest.raises(ValueError):
        training.ArrowBatches(names[0], 2, seed, 1, 2)              # one file given directly cannot feed two ranks


def test_accumulation_is_divided_among_the_ranks():
    with pytest.raises(ValueError) as e:
        training.accumulation_per_rank(16, 3)
    assert "16" in str(e.value) and "3" in str(e.value)
    assert training.accumulation_per_rank(16, 8) == 2
    assert training.accumulation_per_rank(16, 1) == 16 and training.accumulation_per_rank(4, 4) == 1


def test_log_interval_backend_and_share_gpu_flags(capfd):
    a = training.parse_args(REQUIRED)
    assert a.log_interval == 0 and a.backend == "nccl" and a.share_gpu is False
    a = training.parse_args(REQUIRED + ["--log-interval", "5", "--backend", "gloo", "--share-gpu"])
    assert (a.log_interval, a.backend, a.share_gpu) == (5, "gloo", True)
    with pytest.raises(SystemExit) as e:
        training.parse_args(REQUIRED + ["--backend", "mpi"])
    assert e.value.code == 2 and "--backend" in capfd.readouterr().err
    doc = " ".join(training.__doc__.split())
    assert "torchrun" in doc and "No DDP" not in doc


def test_rank_reduce_kernel_uses_no_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    csrc = os.path.join(ROOT, "mapf_gpt_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(csrc, "train.hip"), "-o", str(tmp_path / "train.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            kernels[cur] = int(m.group(1))
    new = {k: v for k, v in kernels.items() if "rank_reduce_kernel" in k}
    assert len(new) == 1, sorted(kernels)
    assert all(v == 0 for v in new.values()), new
    # slab_reduce_kernel keeps its own instance: the rank sum is a separate kernel, not a branch of it
    assert any("slab_reduce_kernel" in k for k in kernels)
