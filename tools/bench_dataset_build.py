"""Stage times of the dataset builder's device path on one GPU.

    python tools/bench_dataset_build.py [--rows 4194304] [--runs 10] [--warmup 2] [--out report.json]

Rows: `--rows` rows of seeded bytes in [0, 67), half of them duplicates of the other half, in shuffled order; labels with the
label-5 share of tests/golden/ds_maze.npz (64 / 220).  Per stage (the library's event hooks around each kernel class) and for the
whole DedupSet.filter_and_balance (device events around the call, which includes its one host synchronisation): the median
over `--runs` runs after `--warmup`, and GB/s by algorithmic bytes -- 256 B read per row in the hash pass, 2 x 256 B per
compared row in classify, 256 B read + 256 B written per gathered row.  Two yardsticks from the same run: a device-to-device copy
of the same bytes, and the reference's method (hashlib.sha256(row.tobytes()) into a python set, generate_dataset.py:43-79) on the
first 200 000 rows on the host.  Also the wall time of building the end-to-end test's shards through the device path and through
the host-list path of ObservationGenerator.generate_observations.  Prints one JSON line.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mapf_gpt_amd import _lib  # noqa: E402
from mapf_gpt_amd.dataset_build import DedupSet, build_shards  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def shard_build_wall(tokenize):
    golden = os.path.join(ROOT, "tests", "golden")
    with tempfile.TemporaryDirectory() as d:
        files, maps = [], {}
        for kind, name in (("random", "ds_random"), ("mazes", "ds_maze")):
            g = np.load(os.path.join(golden, name + ".npz"))
            rec = {"metrics": {"CSR": 1.0, "made_actions": g["made_actions"].tolist(), "init_positions": g["init_positions"].tolist()},
                   "env_grid_search": {"map_name": "map_" + kind}}
            maps[kind] = {"map_" + kind: "\n".join("".join("#" if v else "." for v in row) for row in g["grid"][5:-5, 5:-5])}
            files.append(os.path.join(d, f"{kind}-seed-0.json"))
            with open(files[-1], "w") as f:
                json.dump([rec, rec], f)
        times = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            build_shards(maps["mazes"], maps["random"], files, os.path.join(d, "chunk"), 10 ** 6, seed=0, tokenize=tokenize)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return statistics.median(times[1:]) * 1e3


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=4194304)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    _lib.require_gpu()
    n, half = a.rows, a.rows // 2
    g = torch.Generator(device="cuda").manual_seed(0)
    distinct = torch.randint(0, 67, (half, 256), dtype=torch.uint8, device="cuda", generator=g)
    rows = torch.cat([distinct, distinct[: n - half]])[torch.randperm(n, device="cuda", generator=g)].contiguous()
    del distinct
    u = torch.rand(n, device="cuda", generator=g)
    labels = torch.where(u < 64.0 / 220.0, torch.full_like(u, 5), torch.floor((u * 7919.0) % 5.0)).to(torch.int8)
    ds = DedupSet(n)

    per_stage, whole, stats = {}, [], None
    for it in range(a.warmup + a.runs):
        _lib.prof_reset()
        _lib.prof_enable(True)
        ms, (x, y, stats) = event_ms(lambda: ds.filter_and_balance(rows, labels))
        prof = _lib.prof_read()
        _lib.prof_enable(False)
        kept = int(x.shape[0])
        del x, y
        if it >= a.warmup:
            whole.append(ms)
            for k, (t, launches) in prof.items():
                per_stage.setdefault(k, []).append(t)
    n_first = n - stats["duplicates"]
    # without the hooks: the figure a user sees
    plain = [event_ms(lambda: ds.filter_and_balance(rows, labels))[0] for _ in range(a.warmup + a.runs)][a.warmup:]

    dst = torch.empty_like(rows)
    copy = [event_ms(lambda: dst.copy_(rows))[0] for _ in range(a.warmup + a.runs)][a.warmup:]
    del dst

    host = rows[:200000].cpu().numpy().view(np.int8)
    t0 = time.perf_counter()
    seen = set()
    for r in host:
        seen.add(hashlib.sha256(r.tobytes()).hexdigest())
    sha_s = time.perf_counter() - t0

    med = {k: statistics.median(v) for k, v in per_stage.items()}
    bytes_of = {"ds_row_hash": 256 * n, "ds_classify": 2 * 256 * n, "ds_gather": 512 * (n_first + kept)}
    copy_ms = statistics.median(copy)
    rep = {"rows": n, "bytes": 256 * n, "first_occurrences": n_first, "kept": kept, "stats": stats, "runs": a.runs,
           "stage_ms": {k: round(v, 4) for k, v in med.items()},
           "stage_GBps": {k: round(b / (med[k] * 1e-3) / 1e9, 1) for k, b in bytes_of.items() if k in med},
           "filter_and_balance_ms_with_hooks": round(statistics.median(whole), 3),
           "filter_and_balance_ms": round(statistics.median(plain), 3),
           "filter_and_balance_min_max_ms": [round(min(plain), 3), round(max(plain), 3)],
           "filter_and_balance_rows_per_s": round(n / (statistics.median(plain) * 1e-3)),
           "d2d_copy_ms": round(copy_ms, 4), "d2d_copy_GBps_read_plus_write": round(2 * 256 * n / (copy_ms * 1e-3) / 1e9, 1),
           "hash_ms_per_copy_ms": round(med.get("ds_row_hash", float("nan")) / copy_ms, 3),
           "classify_ms_per_copy_ms": round(med.get("ds_classify", float("nan")) / copy_ms, 3),
           "host_sha256_set_200k_rows_s": round(sha_s, 3), "host_sha256_rows_per_s": round(200000 / sha_s),
           "shards_device_path_ms": round(shard_build_wall("device"), 2), "shards_host_list_path_ms": round(shard_build_wall("host"), 2)}
    line = json.dumps(rep)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
