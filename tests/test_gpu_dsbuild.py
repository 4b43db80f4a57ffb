"""Dataset builder on the device (mapf_gpt_amd/dataset_build.py over mgpt_dedup_* / mgpt_dataset_balance / mgpt_rows_*) against the
goldens of the reference's own functions (tests/golden/dsbuild.npz) and the restatement pinned to them (tests/dsbuild_ref.py)."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from mapf_gpt_amd import _lib
from tests import dsbuild_ref as ref

pytestmark = pytest.mark.gpu
GOLDEN = ref.GOLDEN


def dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a).view(dtype) if a.dtype.itemsize == 1 else a.astype(dtype)).cuda()


def run(ds, rows, labels, keep_known=False):
    """filter_and_balance on host arrays -> (kept indices, kept labels, stats, kept rows), all on the host."""
    x, y = dev(rows, np.uint8), dev(np.asarray(labels, np.int8), np.int8)
    idx, labels_out, stats = ds.filter_and_balance_index(x, y, keep_known)
    idx = idx.cpu().numpy()
    return idx, labels_out.cpu().numpy()[idx], stats


def check(ds, rows, labels, known=None, keep_known=False, tag=None):
    e_idx, e_lab, e_stats = ref.filter_and_balance(rows, labels, known)
    idx, lab, stats = run(ds, rows, labels, keep_known)
    assert np.array_equal(idx, e_idx), tag
    assert np.array_equal(lab, e_lab), tag
    assert stats == e_stats, (tag, stats, e_stats)


_synthetic = {}


def synthetic_rows(n, seed=7):
    """n pairwise distinct rows of seeded bytes in [0, 67)."""
    if (n, seed) not in _synthetic:
        x = np.random.Generator(np.random.PCG64(seed)).integers(0, 67, (n, 256)).astype(np.int8)
        assert len(np.unique(x.view(np.dtype((np.void, 256))).reshape(-1))) == n
        _synthetic[(n, seed)] = x
    return _synthetic[(n, seed)]


@pytest.mark.parametrize("hash_bits", [64, 4, 1])
def test_golden_cases(hash_bits):
    """Every case of the reference's balance_and_filter_tensors; at 4 bits and 1 bit nearly every row shares its hash with a
    different row, so the byte-exact pass decides: the results may not move."""
    from mapf_gpt_amd.dataset_build import DedupSet
    ds = DedupSet(1024, hash_bits=hash_bits)
    for c, case in enumerate(ref.golden_cases()):
        rows = ref.source_rows(case["src"])[0][case["idx"]]
        idx, lab, stats = run(ds, rows, case["labels"], keep_known=case["known"] >= 0)
        assert np.array_equal(idx, case["out_idx"]), c
        assert np.array_equal(lab, case["out_labels"]), c
        assert stats["kept"] == len(idx) and stats["kept"] + stats["discarded"] + stats["duplicates"] == len(rows), c
    # the rows themselves, through the gather
    x, y = dev(rows, np.uint8), dev(case["labels"], np.int8)
    kx, ky, _ = ds.filter_and_balance(x, y)
    e_idx, e_lab, _ = ref.filter_and_balance(rows, case["labels"])
    assert np.array_equal(kx.cpu().numpy().view(np.int8), rows[e_idx]) and np.array_equal(ky.cpu().numpy(), e_lab)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4097])
def test_edge_shapes(n):
    """The edges of 16 lanes per row, four rows per wave, a 256-thread block and the second tile of the scans."""
    from mapf_gpt_amd.dataset_build import DedupSet
    rng = np.random.Generator(np.random.PCG64(n))
    pool, own = ref.source_rows("ds_random")
    ds = DedupSet(n)
    pick = rng.integers(0, len(pool), n)
    check(ds, pool[pick], own[pick], tag="mixed")
    check(ds, pool[pick], rng.integers(0, 6, n).astype(np.int8), tag="uniform labels")
    check(ds, np.repeat(pool[3:4], n, axis=0), rng.integers(0, 6, n).astype(np.int8), tag="all rows identical")
    distinct = synthetic_rows(4097)[:n]
    check(ds, distinct, rng.integers(0, 6, n).astype(np.int8), tag="no duplicates")
    check(ds, distinct, np.full(n, 5, np.int8), tag="every label 5")
    check(ds, pool[pick], np.full(n, 5, np.int8), tag="every label 5, duplicates")
    check(ds, distinct, rng.integers(0, 5, n).astype(np.int8), tag="no label 5")


@pytest.mark.parametrize("hash_bits", [4, 1])
def test_forced_collisions_n257(hash_bits):
    from mapf_gpt_amd.dataset_build import DedupSet
    rng = np.random.Generator(np.random.PCG64(257))
    pool, own = ref.source_rows("ds_random")
    pick = rng.integers(0, len(pool), 257)
    a = run(DedupSet(257, hash_bits=64), pool[pick], own[pick])
    b = run(DedupSet(257, hash_bits=hash_bits), pool[pick], own[pick])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    check(DedupSet(257, hash_bits=hash_bits), pool[pick], own[pick])


@pytest.mark.parametrize("hash_bits", [64, 4])
def test_carry_over(hash_bits):
    """Calls with keep_known=True see the rows of earlier calls: the dedupe flags of two and three calls equal those of one call
    on the concatenation -- at 4 bits too, where first occurrences that are not their hash's representative must be found again."""
    from mapf_gpt_amd.dataset_build import DedupSet
    rng = np.random.Generator(np.random.PCG64(11))
    pool = ref.source_rows("ds_maze")[0]
    rows = pool[rng.integers(0, len(pool), 700)]
    expect = ref.first_occurrences(rows)
    for cuts in ((0, 300, 700), (0, 130, 131, 700)):
        ds = DedupSet(700, hash_bits=hash_bits)
        got = np.concatenate([ds.filter(dev(rows[a:b], np.uint8)).cpu().numpy() for a, b in zip(cuts[:-1], cuts[1:])])
        assert np.array_equal(got.astype(bool), expect), cuts
        assert len(ds) == int(expect.sum())
    one = DedupSet(700, hash_bits=hash_bits).filter(dev(rows, np.uint8)).cpu().numpy()
    assert np.array_equal(one.astype(bool), expect)


def test_capacity_refusal_leaves_the_set_unchanged():
    from mapf_gpt_amd.dataset_build import DedupSet
    rng = np.random.Generator(np.random.PCG64(12))
    pool = ref.source_rows("ds_random")[0]
    rows = pool[rng.integers(0, len(pool), 300)]
    expect = ref.first_occurrences(rows)
    ds = DedupSet(200)
    first = ds.filter(dev(rows[:120], np.uint8)).cpu().numpy()
    held = len(ds)
    with pytest.raises(_lib.MGPTError) as e:
        ds.filter(dev(rows[120:], np.uint8))                    # held + 180 > 200
    assert e.value.code == _lib.ERR_ARG and len(ds) == held
    room = 200 - held
    second = ds.filter(dev(rows[120:120 + room], np.uint8)).cpu().numpy()
    assert np.array_equal(np.concatenate([first, second]).astype(bool), expect[:120 + room])


def test_determinism_at_size():
    """200 000 rows drawn from 50 000: slots are raced for in earnest; two runs give the same flags, and they are numpy's."""
    from mapf_gpt_amd.dataset_build import DedupSet
    rng = np.random.Generator(np.random.PCG64(2024))
    rows = synthetic_rows(50000, seed=9)[rng.integers(0, 50000, 200000)]
    _, first_idx = np.unique(np.ascontiguousarray(rows).view(np.dtype((np.void, 256))).reshape(-1), return_index=True)
    expect = np.zeros(len(rows), np.uint8)
    expect[first_idx] = 1
    x = dev(rows, np.uint8)
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    ds = DedupSet(len(rows))
    a = ds.filter(x, counts).cpu().numpy()
    assert counts.cpu().tolist() == [int(expect.sum()), int(len(rows) - expect.sum()), 0, int(expect.sum())]
    ds.reset()
    b = ds.filter(x).cpu().numpy()
    c = DedupSet(len(rows)).filter(x).cpu().numpy()
    assert np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(a, expect)


def test_select_and_gather_primitives():
    from mapf_gpt_amd.dataset_build import _i64_dev, _workspace, gather_rows
    import ctypes
    rng = np.random.Generator(np.random.PCG64(5))
    for n in (1, 16, 4096, 4097, 12289):
        keep = (rng.random(n) < 0.4).astype(np.uint8)
        for off in (0, 3):                                      # a mask that does not start on a 16-byte boundary
            buf = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
            buf[off:off + n] = torch.as_tensor(keep).cuda()
            k = buf[off:off + n]
            index, count, work = _i64_dev(n, "cuda"), _i64_dev(1, "cuda"), _workspace(n, "cuda")
            _lib.check(_lib.lib().mgpt_rows_select(_lib.ptr(k), n, _lib.ptr(index), _lib.ptr(count), _lib.ptr(work), _lib.stream_ptr()))
            m = int(count.item())
            assert m == int(keep.sum()) and np.array_equal(index[:m].cpu().numpy(), np.flatnonzero(keep)), (n, off)
    rows, labels = synthetic_rows(4097), rng.integers(0, 6, 4097).astype(np.int8)
    perm = rng.permutation(4097)[:1000]
    x, y = gather_rows(dev(rows, np.uint8), dev(labels, np.int8), torch.as_tensor(perm).cuda())
    assert np.array_equal(x.cpu().numpy().view(np.int8), rows[perm]) and np.array_equal(y.cpu().numpy(), labels[perm])


def _to_str(obst):
    return "\n".join("".join("#" if v else "." for v in row) for row in obst)


def _log(name, map_name, twice=False):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    m = {"CSR": 1.0, "made_actions": g["made_actions"].tolist(), "init_positions": g["init_positions"].tolist()}
    if "lifelong_targets" in g:
        m["global_lifelong_targets_xy"] = g["lifelong_targets"].tolist()
    data = [{"metrics": m, "env_grid_search": {"map_name": map_name}}] * (2 if twice else 1)
    return g, {map_name: _to_str(g["grid"][5:-5, 5:-5])}, data


@pytest.mark.parametrize("name", sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "ds_*.npz"))))
def test_tokenizer_rows_stay_on_the_device(name):
    from mapf_gpt_amd.dataset_tokenizer import InputParameters, ObservationGenerator
    g, maps, data = _log(name, "m")
    data = data + [{"metrics": dict(data[0]["metrics"], CSR=0.0), "env_grid_search": {"map_name": "m"}}]      # skipped: not solved
    gen = ObservationGenerator(maps, data, InputParameters(mask_cost2go="mask_cost2go" in g))
    x, y = gen.generate_observations_device(0, 2)
    assert x.is_cuda and x.dtype == torch.uint8 and tuple(x.shape) == g["inputs"].shape and y.is_cuda and y.dtype == torch.int8
    assert np.array_equal(x.cpu().numpy().view(np.int8), g["inputs"]) and np.array_equal(y.cpu().numpy(), g["gt_actions"])
    inputs, gts = gen.generate_observations(0, 2)
    assert np.array_equal(np.stack(inputs), x.cpu().numpy().view(np.int8)) and np.array_equal(np.array(gts), y.cpu().numpy())
    e = gen.generate_observations_device(1, 2)
    assert tuple(e[0].shape) == (0, 256) and tuple(e[1].shape) == (0,)


@pytest.fixture(scope="module")
def logs(tmp_path_factory):
    """A "random" and a "mazes" log, every instance listed twice, and the restatement's survivors per file."""
    d = tmp_path_factory.mktemp("dsbuild")
    out = {"dir": d, "files": [], "maps": {}, "survivors": {}}
    for kind, name in (("random", "ds_random"), ("mazes", "ds_maze")):
        g, maps, data = _log(name, "map_" + kind, twice=True)
        path = str(d / f"{kind}-seed-0.json")
        with open(path, "w") as f:
            json.dump(data, f)
        rows, labels = np.concatenate([g["inputs"]] * 2).astype(np.int8), np.concatenate([g["gt_actions"]] * 2)
        idx, lab, stats = ref.filter_and_balance(rows, labels)
        assert stats["duplicates"] == len(g["inputs"])
        out["files"].append(path)
        out["maps"][kind] = maps
        out["survivors"][kind] = {(rows[i].tobytes(), int(l)) for i, l in zip(idx, lab)}
        assert len(out["survivors"][kind]) == len(idx)
    return out


def _read(prefix):
    from mapf_gpt_amd.scoring import read_arrow
    files = sorted(glob.glob(prefix + "_part_*.arrow"), key=lambda p: int(p.rsplit("_", 1)[1][:-6]))
    xs, ys = zip(*(read_arrow(f) for f in files))
    return files, [len(x) for x in xs], np.concatenate(xs), np.concatenate(ys)


def test_end_to_end_shards(logs):
    from mapf_gpt_amd.dataset_build import build_shards, elements_to_pick, shard_bounds
    from mapf_gpt_amd.training import ArrowBatches
    d, mz, rd = logs["dir"], logs["survivors"]["mazes"], logs["survivors"]["random"]

    def build(tag, desired, seed, **kw):
        os.makedirs(str(d / tag), exist_ok=True)
        prefix = str(d / tag / "chunk")
        rep = build_shards(logs["maps"]["mazes"], logs["maps"]["random"], logs["files"], prefix, desired, seed=seed, **kw)
        return prefix, rep[0]

    # desired_size >= everything: the union of the per-file survivors, each once
    prefix, rep = build("all0", 10 ** 6, 0, files_per_chunk=3)
    files, sizes, x, y = _read(prefix)
    pairs = [(r.tobytes(), int(l)) for r, l in zip(x, y)]
    assert len(pairs) == len(set(pairs)) == len(mz) + len(rd) and set(pairs) == mz | rd
    assert sizes == [b - a for a, b in shard_bounds(len(pairs), 3)] and rep["rows"] == len(pairs)
    assert [f["kind"] for f in rep["files"]] == ["mazes", "random"] and [f["kept"] for f in rep["files"]] == [len(mz), len(rd)]
    # the same seed: the same bytes on disk; another seed: the same rows in another order
    prefix_b, _ = build("all0b", 10 ** 6, 0, files_per_chunk=3)
    for fa, fb in zip(files, _read(prefix_b)[0]):
        assert open(fa, "rb").read() == open(fb, "rb").read()
    prefix_c, _ = build("all1", 10 ** 6, 1, files_per_chunk=3)
    _, _, xc, yc = _read(prefix_c)
    assert sorted(pairs) == sorted((r.tobytes(), int(l)) for r, l in zip(xc, yc)) and not np.array_equal(x, xc)
    # a smaller desired_size: the pick arithmetic per group, rows of the right file, none twice
    desired = 101
    prefix_s, rep_s = build("small", desired, 0, maze_ratio=0.7, files_per_chunk=10)
    _, sizes_s, xs, ys = _read(prefix_s)
    pairs_s = [(r.tobytes(), int(l)) for r, l in zip(xs, ys)]
    want_m, want_r = int(desired * 0.7), desired - int(desired * 0.7)
    assert elements_to_pick([len(mz)], want_m) == ([want_m], want_m)
    assert [f["picked"] for f in rep_s["files"]] == [want_m, want_r]
    assert len(pairs_s) == len(set(pairs_s)) == desired
    assert sum(p in mz for p in pairs_s) == want_m and sum(p in rd for p in pairs_s) == want_r
    assert sizes_s == [10] * 9 + [11]
    # the training loader reads what was written
    xb, tb = next(iter(ArrowBatches(str(d / "all0"), 32)))
    assert xb.shape == (32, 256) and tb.shape == (32, 256) and (tb[:, :-1] == -1).all() and ((tb[:, -1] >= 0) & (tb[:, -1] <= 4)).all()
