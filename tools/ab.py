"""tools/ab.py -- A/B of builds of the library inside ONE visit of a GPU machine: the schedule, the stop rule and the band (DESIGN
sections 27 and 28).  Machines and visits differ by more than most kernel changes, so builds are only compared run against run in one visit.

    python tools/ab.py --lib p=PATH --lib t=PATH [--lib c=PATH] --schedule "p t p t  p c p c" \\
                       --limit SECONDS --out FILE.jsonl [--visit N] -- <command ...>
    python tools/ab.py --summary FILE.jsonl --ref p,c --test t [--key ms_per_step] [--key kernel_ms_per_step.gpt_attention]
                       [--witness-key kernel_ms_per_step.gpt_mlp_fused]

Running.  The libraries are files that `python -m mapf_gpt_amd.build --out` wrote (p = the parent commit's, t = this tree's, c = a byte
copy of p, by convention).  For every label of the schedule, in order and strictly one after the other, <command> runs as a fresh child
process under `timeout -k 10 <limit>` with MGPT_LIB_PATH naming that label's file; nothing is ever copied over the installed library, and
this tool itself imports neither torch nor the library.  The last JSON line of the child's stdout is its result.  One record per run is
appended to --out: visit, run (1, 2, ... in schedule order), library (the label), ms_per_step and kernel_ms_per_step of the result, tool
(the command), and exit_status, sha256 (of the library file: a copy is a copy when the hashes say so), path (as given) and failed.

The stop rule.  A run has failed when the child's exit status is not 0 (124 / 137 from the limit, 134, 139, a negative status from a
signal, anything else), when its stderr contains "illegal memory access", or when its stdout holds no JSON line.  The failed record is
written with the reason in `failed`, NOTHING MORE IS STARTED, and the tool exits with status 1 after saying what failed.  There is no retry.

The summary.  Records are grouped by (visit, tool); per group and key the runs are printed in order.  The band is the minimum and maximum of
the --ref runs of the schedule's reference half, and the verdict is the highest --test run against it: `within`, or `above by X`.  No
threshold is built in; the band is whatever was measured.  A --witness-key is a class whose code is byte-identical in every library: it
gets the same treatment and shows what the schedule alone does.  --test may be given more than once (a label may hold a comma).
The halves: records do not say which half of the schedule a run belongs to, so it is derived from the run order -- the runs of a group,
in order, are cut into two halves of equal length, and the reference half is the one with no --test run in it (DESIGN section 27:
"p t p t" then "p c p c", or "t p t p" then "c p c p").  A group that cannot be cut that way is reported and given no verdict.
"""
import argparse
import hashlib
import json
import os
import shlex
import subprocess
import sys

FAULT_TEXT = "illegal memory access"


# ---- pure functions (tests/test_tools_cpu.py) ----
def parse_schedule(text, labels):
    """"p t p t  p c p c" -> ["p", "t", ...]; every label must be one of `labels`."""
    order = text.split()
    unknown = sorted(set(order) - set(labels))
    if not order or unknown:
        raise ValueError(f"schedule {text!r}: " + (f"no --lib for {unknown}" if unknown else "empty"))
    return order


def last_json_line(stdout):
    """The last line of `stdout` that parses as a JSON object, or None."""
    for line in reversed(stdout.splitlines()):
        line = line.strip()
        if line.startswith("{"):
            try:
                return json.loads(line)
            except ValueError:
                continue
    return None


def failure(exit_status, stdout, stderr):
    """Why this run ends the visit, or None."""
    if exit_status != 0:
        return f"exit status {exit_status}"
    if FAULT_TEXT in stderr:
        return f"stderr contains '{FAULT_TEXT}'"
    if last_json_line(stdout) is None:
        return "no JSON line on stdout"
    return None


def lookup(record, key):
    """record["a"]["b"] for key "a.b"; None where a level is missing."""
    for part in key.split("."):
        record = record.get(part) if isinstance(record, dict) else None
    return record


def groups(records):
    """{(visit, tool): records in file order}, keys in order of first appearance."""
    out = {}
    for r in records:
        out.setdefault((r["visit"], r["tool"]), []).append(r)
    return out


def band(records, ref, test, key):
    """Verdict of one (visit, tool) group on one key.  -> dict(runs=[(label, value)], lo, hi, highest, verdict) with verdict "within" or
    "above by X", or dict(runs=..., verdict=None, why=...) when the group has no test run or its halves cannot be told apart."""
    runs = [(r["library"], lookup(r, key)) for r in records if not r.get("failed") and lookup(r, key) is not None]
    out = {"runs": runs}
    half = len(runs) // 2
    halves = [h for h in (runs[:half], runs[half:]) if not any(label in test for label, _ in h)]
    tested = [v for label, v in runs if label in test]
    if not tested or len(runs) % 2 or len(halves) != 1:
        return dict(out, verdict=None, why="no --test run" if not tested else "no half of the runs is free of --test runs")
    reference = [v for label, v in halves[0] if label in ref]
    if not reference:
        return dict(out, verdict=None, why="no --ref run in the reference half")
    lo, hi, highest = min(reference), max(reference), max(tested)
    return dict(out, lo=lo, hi=hi, highest=highest, verdict="within" if highest <= hi else f"above by {highest - hi:.3f}")


def summary_lines(records, ref, test, keys, witness_keys=()):
    lines = []
    for (visit, tool), recs in groups(records).items():
        shown = False
        for key, witness in [(k, False) for k in keys] + [(k, True) for k in witness_keys]:
            b = band(recs, ref, test, key)
            if not b["runs"]:
                continue
            if not shown:
                lines.append(f"visit {visit}: {tool}")
                shown = True
            runs = ", ".join(f"{label} {value:.3f}" for label, value in b["runs"])
            lines.append(f"  {key}{' (witness: identical code)' if witness else ''}: {runs}")
            if b["verdict"] is None:
                lines.append(f"    no verdict: {b['why']}")
            else:
                lines.append(f"    band {b['lo']:.3f}-{b['hi']:.3f}, highest test run {b['highest']:.3f}: {b['verdict']}")
    return lines


# ---- the runner ----
def sha256_file(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for block in iter(lambda: f.read(1 << 20), b""):
            h.update(block)
    return h.hexdigest()


def run_visit(libs, order, limit, out_path, visit, command):
    hashes = {label: sha256_file(path) for label, path in libs.items()}
    absolute = {label: os.path.abspath(path) for label, path in libs.items()}      # the child may change directory; the record keeps the path as given
    tool = " ".join(shlex.quote(c) for c in command)
    for run, label in enumerate(order, 1):
        r = subprocess.run(["timeout", "-k", "10", str(limit), *command], env=dict(os.environ, MGPT_LIB_PATH=absolute[label]),
                           stdin=subprocess.DEVNULL, capture_output=True, text=True, errors="replace")
        result = last_json_line(r.stdout) or {}
        why = failure(r.returncode, r.stdout, r.stderr)
        kernels = result.get("kernel_ms_per_step") or {}
        ms = result.get("ms_per_step")
        record = {"visit": visit, "run": run, "library": label, "ms_per_step": None if ms is None else round(ms, 3),
                  "kernel_ms_per_step": {k: round(v, 3) for k, v in kernels.items()}, "tool": tool,
                  "exit_status": r.returncode, "sha256": hashes[label], "path": libs[label], "failed": why}
        with open(out_path, "a") as f:
            f.write(json.dumps(record) + "\n")
        print(f"run {run} {label}: " + (f"FAILED, {why}" if why else f"ms_per_step {record['ms_per_step']}"), file=sys.stderr, flush=True)
        if why:
            sys.stderr.write(r.stderr[-4000:])
            print(f"ab.py: visit {visit} run {run} ({label}, {libs[label]}) failed: {why}; nothing more is started "
                  f"({len(order) - run} runs of the schedule left out)", file=sys.stderr)
            return 1
    return 0


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    command = []
    if "--" in argv:
        at = argv.index("--")
        argv, command = argv[:at], argv[at + 1:]
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", action="append", default=[], metavar="LABEL=PATH")
    ap.add_argument("--schedule")
    ap.add_argument("--limit", type=int, help="seconds per run")
    ap.add_argument("--out")
    ap.add_argument("--visit", type=int, default=1)
    ap.add_argument("--summary", metavar="FILE.jsonl")
    ap.add_argument("--ref", default="", help="comma-separated labels of the reference runs")
    ap.add_argument("--test", action="append", default=[], help="label of the library under test (repeatable)")
    ap.add_argument("--key", action="append", default=[])
    ap.add_argument("--witness-key", action="append", default=[])
    a = ap.parse_args(argv)
    if a.summary:
        if not a.ref or not a.test:
            ap.error("--summary needs --ref and --test")
        with open(a.summary) as f:
            records = [json.loads(line) for line in f if line.strip()]
        print("\n".join(summary_lines(records, a.ref.split(","), a.test, a.key or ["ms_per_step"], a.witness_key)))
        return 0
    if not (a.lib and a.schedule and a.limit and a.out and command):
        ap.error("a visit needs --lib, --schedule, --limit, --out and a command after --")
    libs = {}
    for item in a.lib:
        label, _, path = item.partition("=")
        if not label or not os.path.isfile(path):
            ap.error(f"--lib {item}: LABEL=PATH of an existing file")
        libs[label] = path
    try:
        order = parse_schedule(a.schedule, libs)
    except ValueError as e:
        ap.error(str(e))
    return run_visit(libs, order, a.limit, a.out, a.visit, command)


if __name__ == "__main__":
    sys.exit(main())
