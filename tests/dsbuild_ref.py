"""Numpy restatement of the dataset builder's semantics, written from that text and
pinned against tests/golden/dsbuild.npz (outputs of the reference's own functions) by tests/test_dsbuild_cpu.py.  The GPU tests
use it for shapes the goldens do not hold."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def first_occurrences(rows, known=None):
    """Step 1.  rows [n, 256] (any one-byte dtype); known: a set of row bytes carried over (updated in place) or None.
    -> bool [n]: True where no earlier row, and no known row, has the same 256 bytes."""
    known = set() if known is None else known
    first = np.zeros(len(rows), bool)
    for i, r in enumerate(np.ascontiguousarray(rows)):
        b = r.tobytes()
        if b not in known:
            known.add(b)
            first[i] = True
    return first


def balance(first, labels):
    """Step 2 over the rows with first[i]: -> (keep bool [n], labels_out int8 [n] with 5 turned into 0, stats)."""
    first, labels = np.asarray(first, bool), np.asarray(labels).astype(np.int64)
    surv = np.flatnonzero(first)
    n = len(surv)
    counts = np.bincount(labels[surv], minlength=6)
    z, n5 = int(counts[0] + counts[5]), int(counts[5])
    k = 0
    while not (k == n5 or (z - k) <= (n - k) // 5):
        k += 1
    keep = first.copy()
    fives = surv[labels[surv] == 5]
    if k:
        keep[fives[len(fives) - k:]] = False              # the k label-5 survivors with the highest indices
    out = labels.copy()
    out[out == 5] = 0
    made = [int(c) for c in counts[:5]] + [n5 - k]          # as the reference prints actions_made: only [5] is decremented
    stats = {"discarded": k, "duplicates": int(len(first) - n), "kept": n - k, "actions_made": made}
    return keep, out.astype(np.int8), stats


def filter_and_balance(rows, labels, known=None):
    """Steps 1 + 2: -> (indices of the kept rows, increasing; their labels; stats)."""
    keep, out, stats = balance(first_occurrences(rows, known), labels)
    idx = np.flatnonzero(keep)
    return idx, out[idx], stats


def elements_to_pick(sizes, desired):
    """Step 4: -> (picks per file, total picked)."""
    total = sum(sizes)
    desired = min(int(desired), total)
    picks = [int(s * desired / total) if total else 0 for s in sizes]
    while sum(picks) < desired:
        for f, s in enumerate(sizes):
            if sum(picks) == desired:
                break
            if picks[f] < s:
                picks[f] += 1
    return picks, desired


_sources = {}


def source_rows(name):
    """(inputs int8 [N, 256], gt_actions int8 [N]) of a ds_* golden, loaded once."""
    if name not in _sources:
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        _sources[name] = (np.ascontiguousarray(g["inputs"].astype(np.int8)), g["gt_actions"].astype(np.int8))
    return _sources[name]


_golden = None


def golden_cases():
    """-> list of dicts {src, idx, labels, out_idx, out_labels, known} from tests/golden/dsbuild.npz, loaded once."""
    global _golden
    if _golden is None:
        g = np.load(os.path.join(GOLDEN, "dsbuild.npz"))
        io, oo = g["in_off"], g["out_off"]
        _golden = [{"src": str(g["case_src"][c]), "known": int(g["case_known"][c]),
                    "idx": g["in_idx"][io[c]:io[c + 1]].astype(np.int64), "labels": g["in_labels"][io[c]:io[c + 1]],
                    "out_idx": g["out_idx"][oo[c]:oo[c + 1]].astype(np.int64), "out_labels": g["out_labels"][oo[c]:oo[c + 1]]}
                   for c in range(len(io) - 1)]
    return _golden


def golden_picks():
    """-> list of (sizes, total, picks, count)."""
    g = np.load(os.path.join(GOLDEN, "dsbuild.npz"))
    po = g["pick_off"]
    return [([int(v) for v in g["pick_sizes"][po[p]:po[p + 1]]], int(g["pick_total"][p]),
             [int(v) for v in g["pick_picks"][po[p]:po[p + 1]]], int(g["pick_count"][p])) for p in range(len(po) - 1)]
