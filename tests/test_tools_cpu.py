"""CPU checks of the A/B tooling: a variant library is loaded by path (MGPT_LIB_PATH) and never replaces the installed one,
`build(out=...)` leaves the installed build alone, tools/ab.py keeps its schedule and stops at the first failed run, and its band
reproduces the table of DESIGN section 27 from the recorded runs."""
import hashlib
import importlib.util
import json
import os
import shutil
import subprocess
import sys

import pytest

from mapf_gpt_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AB = os.path.join(ROOT, "tools", "ab.py")
RECORDED = os.path.join(ROOT, "profiles", "forward_headers_ab.jsonl")


def load_ab():
    spec = importlib.util.spec_from_file_location("ab_tool", AB)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sha256(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def python_child(code, lib_path, timeout=120):
    """`python -c code` from the repository root; lib_path None = MGPT_LIB_PATH unset."""
    env = {k: v for k, v in os.environ.items() if k != "MGPT_LIB_PATH"}
    if lib_path is not None:
        env["MGPT_LIB_PATH"] = lib_path
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


# ---- MGPT_LIB_PATH ----
ABI = "from mapf_gpt_amd import _lib; print(_lib.lib().mgpt_abi_version())"


def test_override_loads_a_copy(tmp_path):
    copy = str(tmp_path / "lib_copy.so")
    shutil.copyfile(build.build(), copy)
    r = python_child(ABI, copy)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip() == "1003"
    assert f"mapf_gpt_amd: library from MGPT_LIB_PATH={copy}" in r.stderr.splitlines()


def test_override_pointing_nowhere_raises(tmp_path):
    build.build()                                          # the installed library exists: it must not be used in the other's place
    r = python_child(ABI, str(tmp_path / "missing.so"))
    assert r.returncode != 0 and r.stdout.strip() == ""
    assert "ImportError" in r.stderr and "MGPT_LIB_PATH" in r.stderr and str(tmp_path / "missing.so") in r.stderr


@pytest.mark.parametrize("value", [None, ""], ids=["unset", "empty"])
def test_override_unset_is_the_installed_path(value):
    build.build()
    r = python_child("from mapf_gpt_amd import _lib; _lib.lib(); print(_lib.LIB_PATH)", value)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip() == build.LIB
    assert "MGPT_LIB_PATH" not in r.stderr


# ---- build(out=...) ----
def test_variant_build_leaves_the_installed_library_alone(tmp_path, monkeypatch):
    import ctypes

    import torch  # noqa: F401  (the HIP runtime the variant binds to, as in mapf_gpt_amd/_lib.py)
    lib = build.build()
    stamp = os.path.join(build.BUILD, "stamp")
    before = (sha256(lib), os.stat(lib).st_mtime_ns, open(stamp).read(), os.stat(stamp).st_mtime_ns, sorted(os.listdir(build.BUILD)))
    normal, _ = build.compile_command("prof.hip")

    commands = []
    real_run = subprocess.run

    def recording_run(cmd, *args, **kwargs):
        commands.append(list(cmd))
        return real_run(cmd, *args, **kwargs)
    monkeypatch.setattr(build.subprocess, "run", recording_run)
    monkeypatch.setattr(build, "SOURCES", ["prof.hip"])    # one small unit: it holds mgpt_abi_version and needs no other
    csrc = tmp_path / "other" / "mapf_gpt_amd" / "csrc"     # "another checkout": the unit, its header and the public header
    os.makedirs(csrc)
    os.makedirs(tmp_path / "other" / "include")
    for name in ("prof.hip", "common.h", "device_mem.h"):
        shutil.copyfile(os.path.join(build.CSRC, name), csrc / name)
    shutil.copyfile(os.path.join(ROOT, "include", "mapf_gpt_amd.h"), tmp_path / "other" / "include" / "mapf_gpt_amd.h")
    out = str(tmp_path / "variant" / "lib_v.so")
    os.makedirs(tmp_path / "variant")
    assert build.build(out=out, csrc=str(csrc), extra_flags=("-DMGPT_SOME_SWITCH=2",)) == out
    monkeypatch.undo()

    after = (sha256(lib), os.stat(lib).st_mtime_ns, open(stamp).read(), os.stat(stamp).st_mtime_ns, sorted(os.listdir(build.BUILD)))
    assert after == before
    assert ctypes.CDLL(out).mgpt_abi_version() == 1003
    assert os.path.exists(out + ".build/prof.o")

    compile_cmd, link_cmd = commands
    assert link_cmd[link_cmd.index("-o") + 1] == out
    # the variant's compile command is the normal build's but for the object, the source directory and the extra flags
    assert "-DMGPT_SOME_SWITCH=2" in compile_cmd

    def neutral(cmd):
        cmd = [c for c in cmd if c != "-DMGPT_SOME_SWITCH=2"]
        o, c = cmd.index("-o"), cmd.index("-c")
        cmd[o + 1] = os.path.basename(cmd[o + 1])
        cmd[c + 1] = os.path.basename(cmd[c + 1])
        return cmd
    assert neutral(compile_cmd) == neutral(normal)
    assert os.path.dirname(compile_cmd[compile_cmd.index("-c") + 1]) == str(csrc)
    with pytest.raises(ValueError):
        build.build(extra_flags=("-DMGPT_SOME_SWITCH=2",))   # a variant never lands on the installed path


# ---- tools/ab.py ----
# the fake command: appends the MGPT_LIB_PATH it sees to the counter file (one line per process started), then behaves as told
FAKE = r"""
import json, os, sys, time
counter, mode = sys.argv[1], sys.argv[2]
with open(counter, "a") as f:
    f.write(os.environ["MGPT_LIB_PATH"] + "\n")
start = sum(1 for _ in open(counter))
print("some output before the result")
if start == 3 and mode == "segv":
    sys.exit(139)
if start == 3 and mode == "sleep":
    time.sleep(60)
if start == 3 and mode == "fault":
    sys.stderr.write("HIP error: an illegal memory access was encountered\n")
print(json.dumps({"ms_per_step": 90.0 + start, "kernel_ms_per_step": {"gpt_attention": 40.0 + start}, "lib_seen": os.environ["MGPT_LIB_PATH"]}))
"""


@pytest.fixture()
def fake_libs(tmp_path):
    paths = {"p": tmp_path / "lib_p.so", "t": tmp_path / "lib_t.so", "c": tmp_path / "lib_c.so"}
    paths["p"].write_bytes(b"parent build")
    paths["t"].write_bytes(b"this build")
    shutil.copyfile(paths["p"], paths["c"])
    return {k: str(v) for k, v in paths.items()}


def run_ab(tmp_path, libs, mode, limit):
    out, counter = tmp_path / "records.jsonl", tmp_path / "starts.txt"
    cmd = [sys.executable, AB, *[a for k, v in libs.items() for a in ("--lib", f"{k}={v}")], "--schedule", "p t p t  p c p c",
           "--limit", str(limit), "--out", str(out), "--visit", "7", "--", sys.executable, "-c", FAKE, str(counter), mode]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    records = [json.loads(line) for line in open(out)]
    return r, records, counter.read_text().splitlines()


def test_ab_runs_the_schedule_in_order(tmp_path, fake_libs):
    r, records, starts = run_ab(tmp_path, fake_libs, "ok", 30)
    assert r.returncode == 0, r.stderr
    order = "p t p t p c p c".split()
    assert [rec["library"] for rec in records] == order and [rec["run"] for rec in records] == list(range(1, 9))
    assert starts == [fake_libs[k] for k in order]         # what each child saw, one process per run
    for rec, label in zip(records, order):
        assert rec["path"] == fake_libs[label] and rec["sha256"] == sha256(fake_libs[label])
        assert rec["visit"] == 7 and rec["exit_status"] == 0 and rec["failed"] is None
        assert rec["ms_per_step"] == 90.0 + rec["run"] and rec["kernel_ms_per_step"] == {"gpt_attention": 40.0 + rec["run"]}
        assert rec["tool"].endswith(" ok") and "-c" in rec["tool"]
    by_label = {rec["library"]: rec["sha256"] for rec in records}
    assert by_label["p"] == by_label["c"] != by_label["t"]  # the copy is provably a copy


@pytest.mark.parametrize("mode, limit", [("segv", 30), ("sleep", 1), ("fault", 30)])
def test_ab_stops_at_the_first_failed_run(tmp_path, fake_libs, mode, limit):
    r, records, starts = run_ab(tmp_path, fake_libs, mode, limit)
    assert r.returncode != 0
    assert len(records) == 3 and len(starts) == 3          # the failed record is written and no fourth process was started
    assert [rec["failed"] for rec in records[:2]] == [None, None] and records[2]["failed"]
    assert records[2]["library"] == "p" and records[2]["run"] == 3
    status = records[2]["exit_status"]
    assert {"segv": status == 139, "sleep": status in (124, 137), "fault": status == 0}[mode], status
    if mode == "fault":
        assert "illegal memory access" in records[2]["failed"]
    assert "nothing more is started" in r.stderr


def test_ab_imports_neither_torch_nor_the_library():
    code = ("import importlib.util, sys; spec = importlib.util.spec_from_file_location('ab_tool', %r); m = importlib.util.module_from_spec(spec); "
            "spec.loader.exec_module(m); assert 'torch' not in sys.modules and 'mapf_gpt_amd' not in sys.modules" % AB)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    src = open(AB).read()
    assert "os.exec" not in src and "execv" not in src


def test_ab_pure_functions():
    ab = load_ab()
    assert ab.parse_schedule("p t p t  p c p c", {"p", "t", "c"}) == "p t p t p c p c".split()
    with pytest.raises(ValueError):
        ab.parse_schedule("p t x", {"p", "t"})
    assert ab.last_json_line('noise\n{"a": 1}\n{"b": 2}\ntrailing\n') == {"b": 2}
    assert ab.last_json_line("no result here\n{broken\n") is None
    for status in (124, 137, 134, 139, -11, 1):
        assert ab.failure(status, '{"ms_per_step": 1}', "")
    assert ab.failure(0, '{"ms_per_step": 1}', "an illegal memory access was encountered")
    assert ab.failure(0, "no json", "")
    assert ab.failure(0, '{"ms_per_step": 1}', "a warning") is None


# DESIGN section 27's table: (visit, --full pass?, key) -> (band, verdict)
PLAIN, FULL = "bench.py --gpus 1 --steps 8 --warmup 2", "bench.py --gpus 1 --steps 8 --warmup 2 --full --no-cpu-baseline --no-secondary --no-tokenizer-leg"
ATT, MLP = "kernel_ms_per_step.gpt_attention", "kernel_ms_per_step.gpt_mlp_fused"
SECTION_27 = [
    (1, PLAIN, "ms_per_step", (93.251, 93.455), 93.470, "above by 0.015"),
    (2, PLAIN, "ms_per_step", (95.935, 96.388), 96.038, "within"),
    (2, FULL, ATT, (43.978, 44.251), 44.171, "within"),
    (2, FULL, MLP, (51.657, 52.176), 52.232, "above by 0.056"),
    (3, PLAIN, "ms_per_step", (95.951, 96.110), 96.194, "above by 0.084"),
    (3, FULL, ATT, (44.031, 44.077), 44.248, "above by 0.171"),
    (3, FULL, MLP, (51.625, 52.001), 52.197, "above by 0.196"),
    (4, PLAIN, "ms_per_step", (94.003, 94.405), 93.966, "within"),
    (4, FULL, ATT, (43.467, 43.499), 43.460, "within"),
    (4, FULL, MLP, (50.854, 51.187), 50.883, "within"),
    (5, PLAIN, "ms_per_step", (94.001, 94.441), 94.323, "within"),
    (5, FULL, ATT, (43.451, 43.524), 43.567, "above by 0.043"),
    (5, FULL, MLP, (50.943, 51.228), 51.232, "above by 0.004"),
]
REF, TEST = ["parent", "copy"], ["this, REFILL arm removed", "this"]


def test_band_reproduces_the_recorded_table():
    ab = load_ab()
    records = [json.loads(line) for line in open(RECORDED)]
    grouped = ab.groups(records)
    for visit, tool, key, (lo, hi), highest, verdict in SECTION_27:
        b = ab.band(grouped[(visit, tool)], REF, TEST, key)
        assert (b["lo"], b["hi"], b["highest"], b["verdict"]) == (lo, hi, highest, verdict), (visit, key, b)
        assert len(b["runs"]) == 8
    assert (1, FULL) not in grouped                         # visit 1 has no --full runs


def test_summary_prints_the_recorded_table():
    cmd = [sys.executable, AB, "--summary", RECORDED, "--ref", "parent,copy", "--test", TEST[0], "--test", TEST[1],
           "--key", "ms_per_step", "--key", ATT, "--witness-key", MLP]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()

    def verdict_of(visit, tool, key):
        at = lines.index(f"visit {visit}: {tool}")
        row = next(i for i in range(at + 1, len(lines)) if lines[i].startswith(f"  {key}"))
        return lines[row], lines[row + 1].strip()
    runs, verdict = verdict_of(1, PLAIN, "ms_per_step")
    assert runs == ("  ms_per_step: parent 93.335, this, REFILL arm removed 93.393, parent 93.405, this, REFILL arm removed 93.470, "
                    "parent 93.455, copy 93.451, parent 93.390, copy 93.251")
    assert verdict == "band 93.251-93.455, highest test run 93.470: above by 0.015"
    assert verdict_of(4, PLAIN, "ms_per_step")[1] == "band 94.003-94.405, highest test run 93.966: within"
    assert verdict_of(3, FULL, ATT)[1] == "band 44.031-44.077, highest test run 44.248: above by 0.171"
    assert verdict_of(4, FULL, ATT)[1] == "band 43.467-43.499, highest test run 43.460: within"
    assert verdict_of(3, FULL, MLP)[0].startswith(f"  {MLP} (witness: identical code): parent 51.969")
