"""Dataset builder without a GPU: the restatement (tests/dsbuild_ref.py) against the goldens written by the reference's own
balance_and_filter_tensors / calculate_elements_to_pick, the shard writer, the pick / mixture / chunk arithmetic and the C ABI's
argument checks."""
import ctypes
import json
import os

import numpy as np
import pytest

from mapf_gpt_amd import _lib, dataset_build as dsb
from tests import dsbuild_ref as ref


@pytest.fixture(scope="module")
def L():
    from mapf_gpt_amd import build
    build.build()
    return _lib.lib()


def test_goldens_hold_what_the_issue_lists():
    cases = ref.golden_cases()
    assert {c["src"] for c in cases} == {"ds_random", "ds_maze", "ds_short", "ds_lifelong"}
    assert min(len(c["idx"]) for c in cases) == 1 and max(len(c["idx"]) for c in cases) == 400
    assert sum(c["known"] >= 0 for c in cases) >= 1
    assert len(ref.golden_picks()) >= 12


def test_restatement_equals_reference_goldens():
    cases = ref.golden_cases()
    known_sets = {}
    for c, case in enumerate(cases):
        rows = ref.source_rows(case["src"])[0][case["idx"]]
        known = None
        if case["known"] >= 0:
            known = known_sets[case["known"]]
        elif any(o["known"] == c for o in cases):
            known = set()
        idx, labels, stats = ref.filter_and_balance(rows, case["labels"], known)
        if known is not None:
            known_sets[c] = known
        assert np.array_equal(idx, case["out_idx"]), c
        assert np.array_equal(labels, case["out_labels"]), c
        assert (np.diff(case["out_idx"]) > 0).all()
        assert stats["kept"] == len(idx) and stats["kept"] + stats["discarded"] + stats["duplicates"] == len(rows)
        assert sum(stats["actions_made"]) == stats["kept"]


def test_pick_arithmetic_equals_reference_goldens():
    for sizes, total, picks, count in ref.golden_picks():
        assert ref.elements_to_pick(sizes, total) == (picks, count), (sizes, total)
        assert dsb.elements_to_pick(sizes, total) == (picks, count), (sizes, total)
        assert sum(picks) == count == min(total, sum(sizes)) and all(p <= s for p, s in zip(picks, sizes))


def test_write_arrow_round_trip_and_schema(tmp_path):
    import pyarrow as pa
    from mapf_gpt_amd.scoring import read_arrow
    x, y = ref.source_rows("ds_random")
    for n in (len(x), 1, 0):
        path = str(tmp_path / f"s{n}.arrow")
        dsb.write_arrow(path, x[:n], y[:n])
        with pa.memory_map(path) as src:
            table = pa.ipc.open_file(src).read_all()
        assert table.schema == pa.schema([("input_tensors", pa.list_(pa.int8())), ("gt_actions", pa.int8())])
        assert table.num_rows == n
        gx, gy = read_arrow(path)
        assert gx.dtype == np.int8 and gx.shape == (n, 256) and np.array_equal(gx, x[:n])
        assert np.array_equal(np.asarray(gy).astype(np.int8), y[:n])
    # uint8 rows (what the device hands over) land as the same bytes
    path = str(tmp_path / "u8.arrow")
    dsb.write_arrow(path, x.view(np.uint8), y)
    assert np.array_equal(read_arrow(path)[0], x)


def test_shard_sizes_follow_the_floor_rule():
    for n, f in ((1003, 10), (7, 10), (0, 3), (40, 4), (41, 1)):
        b = dsb.shard_bounds(n, f)
        assert len(b) == f and b[0][0] == 0 and b[-1][1] == n
        assert all(hi - lo == n // f for lo, hi in b[:-1]) and b[-1][1] - b[-1][0] == n - (f - 1) * (n // f)
        assert all(b[i][1] == b[i + 1][0] for i in range(f - 1))


def test_mixture_classification_and_chunks():
    files = ["/a/Random-seed-1.json", "/a/mazes-seed-0.json", "/b/x_MAZES_2.json", "/a/other.json", "/mazes/plain.json", "/a/random-seed-0.json"]
    mazes, rnd = dsb.files_by_type(files)
    assert mazes == ["/a/mazes-seed-0.json", "/b/x_MAZES_2.json"]                  # the basename decides, not the folder
    assert rnd == ["/a/Random-seed-1.json", "/a/random-seed-0.json"]
    assert dsb.chunk_groups(list("abcdef"), 3) == [["a", "b"], ["c", "d"], ["e", "f"]]
    assert dsb.chunk_groups(list("abcde"), 2) == [["a", "b"], ["c", "d"], ["e"]]   # as the reference slices; it uses the first num_chunks
    with pytest.raises(ValueError):
        dsb.chunk_groups(["a"], 2)
    # maze_desired = int(desired * ratio), random takes the rest
    assert (int(1000 * 0.9), 1000 - int(1000 * 0.9)) == (900, 100)
    assert (int(7 * 0.9), 7 - int(7 * 0.9)) == (6, 1)


def test_split_by_map(tmp_path):
    recs = [{"env_grid_search": {"map_name": m}, "metrics": {"k": i}} for i, m in enumerate(["b", "a", "b", "c", "a"])]
    p = tmp_path / "LaCAM.json"
    p.write_text(json.dumps(recs))
    per = dsb.split_by_map(str(p), str(tmp_path / "temp"))
    assert list(per) == ["b", "a", "c"] and [r["metrics"]["k"] for r in per["b"]] == [0, 2]
    assert json.loads((tmp_path / "temp" / "a.json").read_text()) == per["a"]


def test_new_symbols_exported_and_bound(L):
    for s in ("mgpt_dedup_create", "mgpt_dedup_destroy", "mgpt_dedup_reset", "mgpt_dedup_count", "mgpt_dedup_filter",
              "mgpt_rows_workspace_bytes", "mgpt_dataset_balance", "mgpt_rows_select", "mgpt_rows_gather"):
        assert s in _lib.SYMBOLS and hasattr(L, s), s
    assert L.mgpt_abi_version() == 1003


def test_argument_validation_without_gpu(L):
    h = ctypes.c_void_p()
    assert L.mgpt_dedup_create(None, 16, 64, None) == _lib.ERR_ARG and b"NULL" in L.mgpt_last_error()
    for cap in (0, -5, (1 << 28) + 1):
        assert L.mgpt_dedup_create(ctypes.byref(h), cap, 64, None) == _lib.ERR_ARG, cap
    for bits in (0, -1, 65):
        assert L.mgpt_dedup_create(ctypes.byref(h), 16, bits, None) == _lib.ERR_ARG, bits
        assert b"hash_bits" in L.mgpt_last_error()
    assert not h.value
    assert L.mgpt_dedup_filter(None, None, 1, None, None, None) == _lib.ERR_ARG
    assert L.mgpt_dataset_balance(None, None, 1, None, None, None, None, None) == _lib.ERR_ARG
    assert L.mgpt_rows_select(None, 1, None, None, None, None) == _lib.ERR_ARG
    assert L.mgpt_rows_gather(None, None, 1, None, 1, None, None, None) == _lib.ERR_ARG
    b = ctypes.c_int64(0)
    assert L.mgpt_rows_workspace_bytes(4097, ctypes.byref(b)) == _lib.OK and b.value >= 2 * 40
    assert L.mgpt_rows_workspace_bytes(-1, ctypes.byref(b)) == _lib.ERR_ARG
    assert L.mgpt_dedup_destroy(None) == _lib.OK


def test_dataset_build_kernels_use_no_scratch(tmp_path):
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(root, "mapf_gpt_amd", "csrc", "dataset_build.hip"), "-o", str(tmp_path / "ds.o")],
                       capture_output=True, text=True, timeout=600)
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
    assert len(kernels) == 14 and all("ds_" in k for k in kernels), sorted(kernels)
    assert all(v == 0 for v in kernels.values()), kernels
