"""Writes tests/golden/dsbuild.npz: what the reference's own balance_and_filter_tensors and calculate_elements_to_pick
(dataset/generate_dataset.py:65-133) return on rows of the ds_* goldens drawn with repeats.

    python tests/golden/make_golden_dsbuild.py /path/to/MAPF-GPT

generate_dataset.py is loaded from where it lies; the modules it imports at top level only for its expert step (pogema_toolbox,
experiment_setup, lacam, tokenizer) are replaced by empty stubs, and numpy.random.shuffle is a no-op around every call so that
the output keeps its pre-shuffle order.  The file holds arrays only:
  case_src [cases] (ds_* name), case_known [cases] = -1, or the case whose call ran just before on the same known_hashes set
  in_off [cases + 1] into in_idx (rows of that golden's `inputs`, with repeats) and in_labels
  out_off [cases + 1] into out_idx (position in the case's input of every output row: its first occurrence) and out_labels
  pick_off [picks + 1] into pick_sizes and pick_picks; pick_total, pick_count [picks]
(tests/dsbuild_ref.py: golden_cases, golden_picks read it)
"""
import contextlib
import importlib.util
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def load_reference(root):
    stubs = {"pogema_toolbox": [], "pogema_toolbox.create_env": ["Environment"], "pogema_toolbox.evaluator": ["evaluation"],
             "pogema_toolbox.registry": ["ToolboxRegistry"], "experiment_setup": [], "experiment_setup.create_env": ["create_logging_env"],
             "lacam": [], "lacam.inference": ["LacamInference", "LacamInferenceConfig"], "tokenizer": [],
             "tokenizer.generate_observations": ["ObservationGenerator"], "tokenizer.parameters": ["InputParameters"]}
    for name, attrs in stubs.items():
        m = types.ModuleType(name)
        for a in attrs:
            setattr(m, a, object)
        sys.modules[name] = m
    spec = importlib.util.spec_from_file_location("ref_generate_dataset", os.path.join(root, "dataset", "generate_dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@contextlib.contextmanager
def no_shuffle():
    saved = np.random.shuffle
    np.random.shuffle = lambda x: None
    try:
        yield
    finally:
        np.random.shuffle = saved


def run_case(ref, rows, idx, labels, known):
    tensors = [rows[i] for i in idx]
    with no_shuffle(), contextlib.redirect_stdout(io.StringIO()):
        out_t, out_a = ref.balance_and_filter_tensors(tensors, [int(v) for v in labels], known)
    out_t, out_a = np.asarray(out_t).reshape(-1, 256), np.asarray(out_a, dtype=np.int8).reshape(-1)
    # every output row's first occurrence in the input (the ds_* rows are pairwise distinct, so the source row decides)
    first_pos = {}
    for p, i in enumerate(idx):
        first_pos.setdefault(int(i), p)
    src_of = {rows[i].tobytes(): int(i) for i in set(int(v) for v in idx)}
    out_idx = np.array([first_pos[src_of[t.tobytes()]] for t in out_t], dtype=np.int64)
    assert (np.diff(out_idx) > 0).all(), "output order is not input order"
    return out_idx, out_a


def main(root):
    ref = load_reference(root)
    rng = np.random.Generator(np.random.PCG64(20240917))
    cases = []

    def add(src, idx, labels, known_set=None, known_case=-1):
        out_idx, out_labels = run_case(ref, srcs[src][0], idx, labels, known_set)
        cases.append((src, np.asarray(idx, np.int16), np.asarray(labels, np.int8), out_idx.astype(np.int16), out_labels, known_case))
        return len(cases) - 1

    srcs = {}
    for name in ("ds_random", "ds_maze", "ds_short", "ds_lifelong"):
        g = np.load(os.path.join(HERE, name + ".npz"))
        rows = g["inputs"].astype(np.int8)
        assert len({r.tobytes() for r in rows}) == len(rows), f"{name} holds a duplicate row"
        srcs[name] = (rows, g["gt_actions"].astype(np.int8))

    def labels_for(kind, src, idx):
        if kind == "own":
            return srcs[src][1][idx]
        if kind == "uniform":
            return rng.integers(0, 6, len(idx)).astype(np.int8)
        return rng.choice(np.arange(6), size=len(idx), p=[0.05, 0.05, 0.1, 0.05, 0.05, 0.7]).astype(np.int8)       # label-5-heavy

    for src in srcs:
        total = len(srcs[src][0])
        for pool, n in ((1, 1), (1, 7), (3, 40), (max(2, total // 4), 130), (total, 257), (total, total), (total, 400)):
            pool_rows = rng.permutation(total)[:pool]
            for kind in ("own", "uniform", "heavy5"):
                idx = pool_rows[rng.integers(0, pool, n)]
                add(src, idx, labels_for(kind, src, idx))
        add(src, np.arange(total), srcs[src][1])                                    # no duplicate at all
    # known_hashes carried over two (and a third) calls
    known = set()
    prev = -1
    for n in (150, 200, 90):
        idx = rng.integers(0, 168, n)
        prev = add("ds_random", idx, labels_for("uniform", "ds_random", idx), known, prev)
    off = lambda k: np.cumsum([0] + [len(cs[k]) for cs in cases]).astype(np.int64)
    cat = lambda k: np.concatenate([cs[k] for cs in cases])
    out = {"case_src": np.array([cs[0] for cs in cases]), "case_known": np.array([cs[5] for cs in cases], np.int64),
           "in_off": off(1), "in_idx": cat(1), "in_labels": cat(2), "out_off": off(3), "out_idx": cat(3), "out_labels": cat(4)}

    picks = [([10, 20, 30], 30), ([10, 20, 30], 60), ([10, 20, 30], 100), ([0, 5, 0, 7], 6), ([0, 5, 0, 7], 12), ([1, 1, 1], 2),
             ([7], 3), ([7], 0), ([3, 0, 3], 5), ([100, 1, 1], 51), ([13, 17, 19, 23], 71), ([2, 9, 4], 1), ([5, 5], 11)]
    got_picks, counts = [], []
    for p, (sizes, total) in enumerate(picks):
        data = {f"f{i}": (np.zeros((s, 1), np.int8), np.zeros(s, np.int8)) for i, s in enumerate(sizes)}
        with contextlib.redirect_stdout(io.StringIO()):
            got, count = ref.calculate_elements_to_pick(data, total)
        got_picks.append([got[f"f{i}"] for i in range(len(sizes))])
        counts.append(count)
    out.update({"pick_off": np.cumsum([0] + [len(sz) for sz, _ in picks]).astype(np.int64),
                "pick_sizes": np.concatenate([np.asarray(sz, np.int64) for sz, _ in picks]),
                "pick_total": np.array([t for _, t in picks], np.int64), "pick_picks": np.concatenate([np.asarray(g, np.int64) for g in got_picks]),
                "pick_count": np.array(counts, np.int64)})
    np.savez_compressed(os.path.join(HERE, "dsbuild.npz"), **out)
    print("dsbuild.npz:", len(cases), "cases,", len(picks), "pick cases,", os.path.getsize(os.path.join(HERE, "dsbuild.npz")), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MAPF_GPT_REFERENCE", ""))
