"""Dataset builder: steps 2-3 of the reference's dataset/generate_dataset.py (split the expert log by map, tokenize, drop
duplicate rows, balance the "wait in goal" label, pick a maze / random mixture, shuffle, write .arrow shards) with the rows
kept on the device from the tokenizer until the shard is written.

    python -m mapf_gpt_amd.dataset_build --logs temp/*.json --maps-mazes mazes/maps.yaml --maps-random random/maps.yaml \\
        --out dataset/chunk --desired-size 1000000 [--maze-ratio 0.9 --files-per-chunk 10 --num-chunks 1 --seed 0]

prints one JSON line per chunk (per-file counters, picks, shard sizes) and writes <out>_part_<i>.arrow (<out>_chunk_<c>_part_<i>.arrow with --num-chunks > 1), the files
`python -m mapf_gpt_amd.training` and `mapf_gpt_amd.scoring` read.  Step 1 of that script runs the LaCAM expert under
POGEMA, which is not part of this repository; `python -m mapf_gpt_amd.expert` writes a log of the same shape with the PIBT expert
(PIBT.json); `split_by_map` is its step 2.

`EpisodeStore` + `build_shards_from_store` are the same steps 2-3 with no log file: the store keeps the expert's
device logs as the batches are planned (evaluation(on_expert_batch=store.append)), every map's episodes become rows in one
dataset_tokenizer.tokenize_episodes call per (map, batch), and from there on the code is the one below.  `python -m mapf_gpt_amd.expert
--shards` and `python -m mapf_gpt_amd.ddg --shards` write shards this way; `EpisodeStore(lifelong=True)` and `python -m mapf_gpt_amd.expert
--lifelong-shards` do the same for lifelong (on_target: restart) episodes, whose goal changes along the path.

Shuffles draw from one np.random.Generator(PCG64(seed)) in a fixed order (per file in processing order, then the whole chunk);
the reference draws from numpy's global stream, so orders differ from it seed for seed while the sets of rows do not.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

from . import _lib

STAT_NAMES = ("discarded", "duplicates", "kept")          # generate_dataset.py:96 prints these three, then actions_made
METRIC_CSR = 0                                             # env.METRIC_KEYS: the column of CSR in BatchedExpert.metrics()


def _i64_dev(n, device):
    return torch.empty((n,), dtype=torch.int64, device=device)


def _workspace(n, device):
    b = ctypes.c_int64(0)
    _lib.check(_lib.lib().mgpt_rows_workspace_bytes(int(n), ctypes.byref(b)))
    return torch.empty((b.value,), dtype=torch.uint8, device=device)


def gather_rows(rows, labels, index):
    """(rows[index], labels[index]) through mgpt_rows_gather; index: int64 device tensor."""
    n_out = int(index.shape[0])
    index = index.contiguous()
    out = torch.empty((n_out, 256), dtype=torch.uint8, device=rows.device)
    lab = torch.empty((n_out,), dtype=torch.int8, device=rows.device)
    with _lib.on_device(rows.device):
        _lib.check(_lib.lib().mgpt_rows_gather(_lib.ptr(rows), _lib.ptr(labels), int(rows.shape[0]), _lib.ptr(index), n_out,
                                               _lib.ptr(out), _lib.ptr(lab), _lib.stream_ptr()))
    return out, lab


class DedupSet:
    """The set of rows seen so far (mgpt_dedup_*): exact duplicate filtering on the device, carried over between calls."""

    def __init__(self, capacity_rows, hash_bits=64, device="cuda"):
        _lib.require_gpu()
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.capacity = int(capacity_rows)
        self._h = ctypes.c_void_p()
        with _lib.on_device(self.device):
            _lib.check(_lib.lib().mgpt_dedup_create(ctypes.byref(self._h), self.capacity, int(hash_bits), _lib.stream_ptr()))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                _lib.lib().mgpt_dedup_destroy(h)
            except Exception:
                pass
            self._h = None

    def __len__(self):
        n = ctypes.c_int64(0)
        _lib.check(_lib.lib().mgpt_dedup_count(self._h, ctypes.byref(n)))
        return n.value

    def reset(self):
        with _lib.on_device(self.device):
            _lib.check(_lib.lib().mgpt_dedup_reset(self._h, _lib.stream_ptr()))

    def _rows(self, rows):
        assert rows.dtype == torch.uint8 and rows.dim() == 2 and rows.shape[1] == 256 and rows.device == self.device, \
            "rows: uint8 [n, 256] on the set's device"
        return rows.contiguous()

    def filter(self, rows, counts=None):
        """-> uint8 device tensor [n]: 1 where the row is the first occurrence of its 256 bytes (in the set so far and in
        `rows`); those rows join the set.  counts: optional int64 device tensor [4] (see include/mapf_gpt_amd.h)."""
        rows = self._rows(rows)
        n = int(rows.shape[0])
        first = torch.empty((n,), dtype=torch.uint8, device=self.device)
        if n == 0:
            return first
        with _lib.on_device(self.device):
            _lib.check(_lib.lib().mgpt_dedup_filter(self._h, _lib.ptr(rows), n, _lib.ptr(first),
                                                    _lib.ptr(counts) if counts is not None else None, _lib.stream_ptr()))
        return first

    def filter_and_balance_index(self, rows, labels, keep_known=False):
        """-> (index int64 device [kept]: the kept rows' positions in `rows`, increasing; labels_out int8 device [n]: labels with
        5 turned into 0; stats).  The one host transfer is the ten counters."""
        rows = self._rows(rows)
        n = int(rows.shape[0])
        assert labels.dtype == torch.int8 and tuple(labels.shape) == (n,) and labels.device == self.device, "labels: int8 [n] on the device"
        labels = labels.contiguous()
        if not keep_known:
            self.reset()
        if n == 0:
            return _i64_dev(0, self.device), labels, {"discarded": 0, "duplicates": 0, "kept": 0, "actions_made": [0] * 6}
        first = self.filter(rows)
        keep = torch.empty_like(first)
        labels_out = torch.empty_like(labels)
        scal = _i64_dev(11, self.device)                 # ten counters of the balance pass, then the kept count of the select pass
        work = _workspace(n, self.device)
        index = _i64_dev(max(n, 1), self.device)
        with _lib.on_device(self.device):
            L, s = _lib.lib(), _lib.stream_ptr()
            _lib.check(L.mgpt_dataset_balance(_lib.ptr(first), _lib.ptr(labels), n, _lib.ptr(keep), _lib.ptr(labels_out),
                                              _lib.ptr(scal), _lib.ptr(work), s))
            _lib.check(L.mgpt_rows_select(_lib.ptr(keep), n, _lib.ptr(index), ctypes.c_void_p(scal.data_ptr() + 80), _lib.ptr(work), s))
        h = scal.cpu().tolist()
        if h[9]:
            raise ValueError(f"{h[9]} labels outside 0..5")
        assert h[10] == h[2], (h[10], h[2])
        stats = {"discarded": h[0], "duplicates": h[1], "kept": h[2], "actions_made": h[3:9]}
        return index[:h[2]], labels_out, stats

    def filter_and_balance(self, rows, labels, keep_known=False):
        """= balance_and_filter_tensors (generate_dataset.py:65-98) before its shuffle: -> (rows_kept uint8 [kept, 256], labels_kept
        int8 [kept], stats) on the device, in the order of `rows`.  stats = {"discarded", "duplicates", "kept", "actions_made"}, the four
        things the reference prints (:96).  keep_known=False empties the set first: what the reference's pipeline does per file."""
        index, labels_out, stats = self.filter_and_balance_index(rows, labels, keep_known)
        x, y = gather_rows(self._rows(rows), labels_out, index)
        return x, y, stats


# ---------------------------------------------------------------------------------------------------------------------
# host arithmetic of the pipeline
# ---------------------------------------------------------------------------------------------------------------------
def elements_to_pick(sizes, total_pick_count):
    """= calculate_elements_to_pick (:105-133) on a list of sizes: -> (picks, total actually picked)."""
    sizes = [int(s) for s in sizes]
    total = sum(sizes)
    want = int(total_pick_count)
    if want > total:
        print(f"Warning! Files don't contain enough data to pick {want} elements. Using {total} elements instead", file=sys.stderr)
        want = total
    if total == 0 or want <= 0:
        return [0] * len(sizes), 0
    picks = [int(s * want / total) for s in sizes]
    got = sum(picks)
    while got < want:
        for f, s in enumerate(sizes):
            if got == want:
                break
            if picks[f] < s:
                picks[f] += 1
                got += 1
    return picks, want


def files_by_type(files):
    """= get_files_by_type (:47-54): (maze files, random files), each sorted; the basename decides, case-insensitively."""
    mazes = sorted(f for f in files if "mazes" in os.path.basename(f).lower())
    rnd = sorted(f for f in files if "random" in os.path.basename(f).lower())
    return mazes, rnd


def chunk_groups(files, num_chunks):
    """= generate_chunks (:249-253): consecutive groups of len(files) // num_chunks files (the reference raises on a group size
    of zero; so does this)."""
    size = len(files) // int(num_chunks)
    if size <= 0:
        raise ValueError(f"{len(files)} files cannot be split into {num_chunks} chunks")
    return [files[i:i + size] for i in range(0, len(files), size)]


def shard_bounds(num_samples, files_per_chunk):
    """= :193-197: files_per_chunk ranges of num_samples // files_per_chunk rows, the last one taking the remainder."""
    per = num_samples // files_per_chunk
    return [(i * per, (i + 1) * per if i < files_per_chunk - 1 else num_samples) for i in range(files_per_chunk)]


def arrow_schema():
    import pyarrow as pa
    return pa.schema([("input_tensors", pa.list_(pa.int8())), ("gt_actions", pa.int8())])


def write_arrow(path, inputs, gt_actions):
    """One shard in the reference's format (:188-210): an Arrow IPC file, input_tensors list<int8> (256 per row), gt_actions int8.
    The list column is the flat buffer plus offsets: no python list is made."""
    import pyarrow as pa
    x = np.ascontiguousarray(np.asarray(inputs)).view(np.int8).reshape(-1, 256) if len(inputs) else np.zeros((0, 256), np.int8)
    y = np.ascontiguousarray(np.asarray(gt_actions), dtype=np.int8).reshape(-1)
    assert x.dtype.itemsize == 1 and len(x) == len(y)
    if len(x) * 256 >= 2 ** 31:
        raise ValueError("a list<int8> column has 32-bit offsets: at most 8388607 rows per shard")
    offsets = pa.array(np.arange(0, (len(x) + 1) * 256, 256, dtype=np.int32), type=pa.int32())
    col = pa.ListArray.from_arrays(offsets, pa.array(x.reshape(-1), type=pa.int8()), type=pa.list_(pa.int8()))
    schema = arrow_schema()
    table = pa.Table.from_arrays([col, pa.array(y, type=pa.int8())], schema=schema)
    with open(path, "wb") as f:
        with pa.ipc.new_file(f, schema) as writer:
            writer.write(table)


def split_by_map(result_json, out_dir=None):
    """= split_json (:232-244): the records of one expert log grouped by env_grid_search.map_name, in log order.  -> {map_name:
    [records]}; with out_dir, also written as <out_dir>/<map_name>.json like the reference's temp folder."""
    with open(result_json, "r") as f:
        data = json.load(f)
    per_map = {}
    for d in data:
        per_map.setdefault(d["env_grid_search"]["map_name"], []).append(d)
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        for k, v in per_map.items():
            with open(os.path.join(out_dir, f"{k}.json"), "w") as f:
                json.dump(v, f)
    return per_map


# ---------------------------------------------------------------------------------------------------------------------
# the pipeline
# ---------------------------------------------------------------------------------------------------------------------
def _balance_and_shuffle(rows, labels, file_name, rng, device):
    """What follows the tokenizer for one file's rows: drop duplicates, balance, shuffle (one rng.permutation).
    -> (rows uint8 [kept, 256], labels int8 [kept]) on the device; stats."""
    n = int(rows.shape[0])
    stats = {"file": file_name, "samples": n, "discarded": 0, "duplicates": 0, "kept": 0, "actions_made": [0] * 6}
    if n == 0:
        return rows, labels, stats
    index, labels_out, st = DedupSet(n, device=device).filter_and_balance_index(rows, labels)
    stats.update(st)
    perm = torch.as_tensor(rng.permutation(st["kept"])).to(rows.device)       # step 3: the index list, not the rows, is shuffled
    x, y = gather_rows(rows, labels_out, index[perm])                        # compaction and shuffle in one gather
    return x, y, stats


def _process_file(path, maps, rng, device, tokenize):
    """One log file -> (rows uint8 [kept, 256], labels int8 [kept]) on the device, balanced and in shuffled order; stats."""
    from .dataset_tokenizer import InputParameters, ObservationGenerator
    with open(path, "r") as f:
        data = json.load(f)
    gen = ObservationGenerator(maps, data, InputParameters(), device=device)
    if tokenize == "device":
        rows, labels = gen.generate_observations_device(0, len(data))
    else:                                                   # the host-list path, kept for comparison (tools/bench_dataset_build.py)
        inputs, gts = gen.generate_observations(0, len(data))
        x = np.stack(inputs).view(np.uint8) if inputs else np.zeros((0, 256), np.uint8)
        rows, labels = torch.as_tensor(x).to(device), torch.as_tensor(np.asarray(gts, dtype=np.int8)).to(device)
    return _balance_and_shuffle(rows, labels, os.path.basename(path), rng, device)


def _assemble_chunk(sources, out_prefix, desired_size, maze_ratio, files_per_chunk, rng):
    """= process_files (:143-212) for one chunk over sources = ((files, process, kind) for mazes, then random): process(file) ->
    (rows, labels, stats) balanced and shuffled, drawing from rng.  -> the chunk's report."""
    maze_desired = int(desired_size * maze_ratio)
    random_desired = desired_size - maze_desired
    report = {"out": out_prefix, "files": [], "shards": []}
    parts = []
    for (files, process, kind), want in zip(sources, (maze_desired, random_desired)):
        done = [process(f) for f in files]
        picks, _ = elements_to_pick([int(x.shape[0]) for x, _, _ in done], want)
        for (x, y, st), p in zip(done, picks):
            st.update(kind=kind, picked=p)
            report["files"].append(st)
            if p > 0:
                parts.append((x[:p], y[:p]))                # a file gives its first pick_f rows after its shuffle
    total = sum(int(x.shape[0]) for x, _ in parts)
    if total:
        xs, ys = torch.cat([x for x, _ in parts]), torch.cat([y for _, y in parts])
        perm = torch.as_tensor(rng.permutation(total)).to(xs.device)
        xs, ys = gather_rows(xs, ys, perm)
        inputs, gts = xs.cpu().numpy().view(np.int8), ys.cpu().numpy()    # the one trip of the rows to the host
    else:
        inputs, gts = np.zeros((0, 256), np.int8), np.zeros((0,), np.int8)
    for i, (a, b) in enumerate(shard_bounds(total, files_per_chunk)):
        path = f"{out_prefix}_part_{i}.arrow"
        write_arrow(path, inputs[a:b], gts[a:b])
        report["shards"].append({"path": path, "rows": b - a})
    report["rows"] = total
    return report


def build_chunk(maps_mazes, maps_random, maze_files, random_files, out_prefix, desired_size, maze_ratio=0.9, files_per_chunk=10,
                rng=None, device="cuda", tokenize="device"):
    """= process_files (:143-212) for one chunk.  -> the chunk's report (what the CLI prints)."""
    rng = rng if rng is not None else np.random.Generator(np.random.PCG64(0))
    sources = ((maze_files, lambda f: _process_file(f, maps_mazes, rng, device, tokenize), "mazes"),
               (random_files, lambda f: _process_file(f, maps_random, rng, device, tokenize), "random"))
    return _assemble_chunk(sources, out_prefix, desired_size, maze_ratio, files_per_chunk, rng)


def _chunk_plan(files, out_prefix, num_chunks):
    """generate_chunks (:246-256): [(maze files, random files, output prefix)] of every chunk."""
    maze_files, random_files = files_by_type(list(files))
    if num_chunks == 1:
        return [(maze_files, random_files, out_prefix)]
    mz, rd = chunk_groups(maze_files, num_chunks), chunk_groups(random_files, num_chunks)
    return [(mz[c], rd[c], f"{out_prefix}_chunk_{c}") for c in range(num_chunks)]


def build_shards(maps_mazes, maps_random, log_files, out_prefix, desired_size, maze_ratio=0.9, files_per_chunk=10, num_chunks=1, seed=0,
                 device="cuda", tokenize="device"):
    """Steps 3 of generate_dataset.py (generate_chunks :246-256) over per-map log files.  desired_size is per chunk, as in the
    reference.  One chunk writes <out_prefix>_part_<i>.arrow; with num_chunks > 1, chunk c writes <out_prefix>_chunk_<c>_part_<i>.arrow
    (the reference's chunk_<c>).  -> list of chunk reports."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return [build_chunk(maps_mazes, maps_random, m, r, out, desired_size, maze_ratio, files_per_chunk, rng, device, tokenize)
            for m, r, out in _chunk_plan(log_files, out_prefix, num_chunks)]


class EpisodeStore:
    """The expert's episodes, kept where they were planned, until the shards are built: append(info) takes one batch of
    evaluation(on_expert_batch=...) and keeps its device log once -- first cells, made actions, lengths, CSR and the frame grids, about one
    byte per agent-step -- plus, per map name, the batch's episode indices in log order.  No row exists until rows_of(map) is asked.
    The episodes of a map name in order (batch, then index) are the records of split_by_map's <map_name>.json in order.
    lifelong=True makes it a store of on_target='restart' batches: append() also keeps the expert's
    lifelong_targets(), every episode counts as kept, and rows_of carries the goal pursued at every timestep.  A store is one or the other."""

    def __init__(self, device="cuda", tables=None, mask_cost2go=False, lifelong=False):
        from .dataset_tokenizer import TableCache
        self.device = torch.device(device)
        self.tables = tables if tables is not None else TableCache(device=self.device)
        self.mask_cost2go = bool(mask_cost2go)
        self.lifelong = bool(lifelong)
        self.batches = []                                    # {init, actions, lengths, solved, grids (host)} + lifelong: {targets, n_targets}
        self.per_map = {}                                    # map name -> [(batch index, [episode indices])], in log order

    @staticmethod
    def group_by_map(run_keys):
        """{map_name: [indices into run_keys]} in order of first appearance, indices increasing: split_by_map on one batch."""
        out = {}
        for k, key in enumerate(run_keys):
            out.setdefault(key["map_name"], []).append(k)
        return out

    def append(self, info):
        on_target = info.get("on_target", "nothing")
        if self.lifelong:
            if on_target != "restart":
                raise NotImplementedError(f"EpisodeStore(lifelong=True) keeps lifelong (on_target='restart') episodes only, not on_target={on_target!r}")
            ex = info["expert"]
            log, lens = ex.log()
            targets, n_targets = ex.lifelong_targets()
            self.add_batch(info["run_keys"], info["pos"], log, lens, torch.ones_like(lens, dtype=torch.bool), info["grids"], targets, n_targets)
            return
        if on_target != "nothing":
            raise NotImplementedError("EpisodeStore keeps no per-step goals: lifelong (on_target='restart') episodes go through the JSON log "
                                      "(or a store made with lifelong=True)")
        ex = info["expert"]
        log, lens = ex.log()
        self.add_batch(info["run_keys"], info["pos"], log, lens, ex.metrics()[:, METRIC_CSR] >= 1, info["grids"])

    def add_batch(self, run_keys, init, actions, lengths, solved, grids, targets=None, n_targets=None):
        """One batch given as tensors (append() reads them off a BatchedExpert; mapf_gpt_amd.ddg hands in the teacher's): run_keys
        [n] dicts with `map_name`; init [n, n_agents, 2]; actions int8 [n, n_agents, max_steps]; lengths [n]; solved bool [n] (CSR >= 1);
        grids [n or 1, H, W], the frame every episode ran in.  A lifelong store also takes the batch's target lists (targets int16 [n,
        n_agents, L, 2], n_targets int32 [n, n_agents] or None, as dataset_tokenizer.tokenize_episodes reads them) and keeps every
        episode whatever `solved` says: a lifelong record has no CSR."""
        actions = torch.as_tensor(actions).to(self.device, torch.int8).contiguous()
        n = int(actions.shape[0])
        assert len(run_keys) == n, "one run key per episode"
        if self.lifelong != (targets is not None):
            raise ValueError("a lifelong store takes batches with targets, a default store batches without")
        grids = np.asarray(grids.cpu() if torch.is_tensor(grids) else grids)
        self.batches.append({"init": torch.as_tensor(init).to(self.device, torch.int16).reshape(n, -1, 2).contiguous(),
                             "actions": actions, "lengths": torch.as_tensor(lengths).to(self.device, torch.int32).contiguous(),
                             "solved": (torch.as_tensor(solved).to(self.device) != 0).to(torch.uint8).contiguous(),
                             "grids": grids[None] if grids.ndim == 2 else grids})
        if self.lifelong:
            self.batches[-1]["solved"].fill_(1)
            self.batches[-1]["targets"] = torch.as_tensor(targets).to(self.device, torch.int16).contiguous()
            self.batches[-1]["n_targets"] = None if n_targets is None else torch.as_tensor(n_targets).to(self.device, torch.int32).contiguous()
        for name, idx in self.group_by_map(run_keys).items():
            self.per_map.setdefault(name, []).append((len(self.batches) - 1, idx))

    def map_names(self):
        return list(self.per_map)

    def episodes(self):
        return sum(int(b["actions"].shape[0]) for b in self.batches)

    def solved_rows(self):
        """(solved episodes, their rows) over the whole store: one reduction per batch on the device."""
        ep = rows = 0
        for b in self.batches:
            k = b["solved"] != 0
            per = (b["lengths"].clamp(0, b["actions"].shape[2]).to(torch.int64) + 1) * int(b["actions"].shape[1])
            e, r = torch.stack([k.sum(), (per * k).sum()]).cpu().tolist()
            ep, rows = ep + e, rows + r
        return ep, rows

    def rows_of(self, map_name):
        """-> (rows uint8 [N, 256], labels int8 [N]) on the device: the solved episodes of the map in log order, one
        tokenize_episodes call per batch that has some -- what generate_observations_device makes of <map_name>.json."""
        from .dataset_tokenizer import tokenize_episodes
        xs, ys = [], []
        for bi, idx in self.per_map.get(map_name, []):
            b = self.batches[bi]
            table = self.tables.get(b["grids"][idx[0] % len(b["grids"])])
            x, y, _ = tokenize_episodes(table, b["init"], b["actions"], b["lengths"], b["solved"], idx, self.mask_cost2go,
                                        targets=b.get("targets"), n_targets=b.get("n_targets"))
            xs.append(x)
            ys.append(y)
        if not xs:
            return torch.empty((0, 256), dtype=torch.uint8, device=self.device), torch.empty((0,), dtype=torch.int8, device=self.device)
        return (xs[0], ys[0]) if len(xs) == 1 else (torch.cat(xs), torch.cat(ys))


def build_shards_from_store(store, out_prefix, desired_size, maze_ratio=0.9, files_per_chunk=10, num_chunks=1, seed=0):
    """build_shards over an EpisodeStore: every map name stands for the file <map_name>.json that split_by_map would have written
    (`mazes` / `random` in the name decides the kind, the names are sorted as files_by_type sorts, chunks are cut as chunk_groups cuts),
    its rows come from store.rows_of, and everything after the tokenizer is build_shards' own code drawing from the one rng in the same
    order -- the same .arrow bytes for the same seed.  -> list of chunk reports."""
    rng = np.random.Generator(np.random.PCG64(seed))
    files = {f"{name}.json": name for name in store.map_names()}

    def process(f):
        rows, labels = store.rows_of(files[f])
        return _balance_and_shuffle(rows, labels, f, rng, store.device)

    return [_assemble_chunk(((m, process, "mazes"), (r, process, "random")), out, desired_size, maze_ratio, files_per_chunk, rng)
            for m, r, out in _chunk_plan(list(files), out_prefix, num_chunks)]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--logs", nargs="+", required=True, help="per-map expert logs (json; 'mazes' / 'random' in the file name decides the group)")
    ap.add_argument("--maps-mazes", required=True, help="maps.yaml of the maze maps ({name: map string})")
    ap.add_argument("--maps-random", required=True, help="maps.yaml of the random maps")
    ap.add_argument("--out", required=True, help="output prefix")
    ap.add_argument("--desired-size", type=int, required=True, help="rows per chunk")
    ap.add_argument("--maze-ratio", type=float, default=0.9)
    ap.add_argument("--files-per-chunk", type=int, default=10)
    ap.add_argument("--num-chunks", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    import yaml
    with open(a.maps_mazes, "r") as f:
        maps_mazes = yaml.safe_load(f)
    with open(a.maps_random, "r") as f:
        maps_random = yaml.safe_load(f)
    out_dir = os.path.dirname(a.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    for rep in build_shards(maps_mazes, maps_random, a.logs, a.out, a.desired_size, a.maze_ratio, a.files_per_chunk, a.num_chunks,
                            a.seed, a.device):
        print(json.dumps(rep), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
