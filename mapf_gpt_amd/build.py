"""Build libmapf_gpt_amd.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

    python -m mapf_gpt_amd.build [--force] [--verbose]
    python -m mapf_gpt_amd.build --out PATH [--csrc DIR] [-D...]

One object per .hip translation unit (parallel), then one shared library next to the sources.
The built .so is git-ignored but travels to the GPU box with the snapshot.
--out builds a variant library somewhere else (another checkout's sources, a -D switch) for an A/B: tools/ab.py and
tools/forward_digest.py load it by path (MGPT_LIB_PATH), it never replaces the installed one.
"""
import argparse
import concurrent.futures
import hashlib
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
BUILD = os.path.join(CSRC, "_build")
LIB = os.path.join(CSRC, "libmapf_gpt_amd.so")
SOURCES = ["prof.hip", "tokenizer.hip", "env.hip", "gpt.hip", "gpt_fast.hip", "step.hip", "train.hip", "dataset_build.hip", "expert.hip"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function",
         "-Wno-unused-variable", "-Wno-unused-but-set-variable"]


def _sources(csrc=CSRC):
    return [s for s in SOURCES if os.path.exists(os.path.join(csrc, s))]


def _stamp():
    h = hashlib.sha256()
    for root, _, files in os.walk(CSRC):
        if "_build" in root:
            continue
        for f in sorted(files):
            if f.endswith((".hip", ".h", ".cpp")):
                with open(os.path.join(root, f), "rb") as fh:
                    h.update(f.encode() + fh.read())
    with open(os.path.join(os.path.dirname(HERE), "include", "mapf_gpt_amd.h"), "rb") as fh:
        h.update(fh.read())
    h.update(" ".join(FLAGS).encode())
    return h.hexdigest()


def compile_command(src, csrc=CSRC, build_dir=BUILD, extra_flags=()):
    """(command, object file) of one translation unit; the normal build and a variant differ in nothing else."""
    obj = os.path.join(build_dir, src.replace(".hip", ".o"))
    return [HIPCC] + FLAGS + list(extra_flags) + ["-c", os.path.join(csrc, src), "-o", obj], obj


def _compile(src, verbose, csrc=CSRC, build_dir=BUILD, extra_flags=()):
    cmd, obj = compile_command(src, csrc, build_dir, extra_flags)
    if verbose:
        print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {src}:\n{r.stdout}\n{r.stderr}")
    if verbose and r.stderr.strip():
        print(r.stderr)
    return obj


def _compile_and_link(lib, verbose, csrc=CSRC, build_dir=BUILD, extra_flags=()):
    os.makedirs(build_dir, exist_ok=True)
    srcs = _sources(csrc)
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:
        objs = list(ex.map(lambda s: _compile(s, verbose, csrc, build_dir, extra_flags), srcs))
    cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
    return lib


def build(force=False, verbose=False, out=None, csrc=None, extra_flags=()):
    """The installed library, rebuilt when its sources or flags changed.  With `out`: a variant library at that path -- the same
    translation units, flags and job count, from `csrc` (default: this checkout's; another checkout's mapf_gpt_amd/csrc for its
    build) with `extra_flags` added; its objects go to <out>.build/, and LIB, _build/ and the stamp are not touched."""
    if out is not None:
        out = os.path.abspath(out)
        return _compile_and_link(out, verbose, os.path.abspath(csrc or CSRC), out + ".build", extra_flags)
    if csrc is not None or extra_flags:
        raise ValueError("csrc and extra_flags build a variant library: name its file with out")
    os.makedirs(BUILD, exist_ok=True)
    stamp_file = os.path.join(BUILD, "stamp")
    stamp = _stamp()
    if not force and os.path.exists(LIB) and os.path.exists(stamp_file) and open(stamp_file).read() == stamp:
        return LIB
    _compile_and_link(LIB, verbose)
    with open(stamp_file, "w") as f:
        f.write(stamp)
    return LIB


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--force", action="store_true")
    ap.add_argument("--verbose", "-v", action="store_true")
    ap.add_argument("--out", help="write a variant library to this path and leave the installed one alone")
    ap.add_argument("--csrc", help="with --out: the directory of translation units to build (another checkout's mapf_gpt_amd/csrc)")
    args, extra = ap.parse_known_args(argv)
    bad = [f for f in extra if not f.startswith("-D")]
    if bad:
        ap.error(f"unknown arguments {bad} (only -D... flags are passed on to hipcc)")
    print(build(args.force, args.verbose, args.out, args.csrc, tuple(extra)))


if __name__ == "__main__":
    main()
