"""tools/kernel_digest.py <file.hip> ...  -- one line per kernel of each translation unit: the demangled name, the SHA-256 of that
symbol's bytes in .text, its size, and the compiler's resource report (VGPRs, AGPRs, SGPRs, scratch, LDS, occupancy).

Each file (a name in mapf_gpt_amd/csrc, or a path) is cross-compiled for the device only, with the flags of mapf_gpt_amd/build.py plus
-Rpass-analysis=kernel-resource-usage; no GPU is needed.  The bytes are hashed and the remarks are copied: no instruction is looked at.
Two outputs diffed (one of the parent commit's sources, one of the tree's: --csrc names another source directory) are the "no kernel
moved" check of a refactor of the device headers.  Lines are sorted by name, so a diff is stable under reordering of the sources.
A kernel that takes the address of a global can change its hash, at equal size, when other kernels of the unit change size.

    python tools/kernel_digest.py gpt_fast.hip > new.txt
    python tools/kernel_digest.py --csrc ../parent/mapf_gpt_amd/csrc gpt_fast.hip > old.txt
"""
import argparse
import concurrent.futures
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mapf_gpt_amd.build import CSRC, FLAGS, HIPCC  # noqa: E402

REPORT = (("V", "VGPRs"), ("A", "AGPRs"), ("S", "TotalSGPRs"), ("scratch", "ScratchSize [bytes/lane]"),
          ("lds", "LDS Size [bytes/block]"), ("occ", "Occupancy [waves/SIMD]"))


def remarks(stderr):
    """{mangled kernel name: {remark key: value}} from the kernel-resource-usage remarks."""
    out, cur = {}, None
    for line in stderr.splitlines():
        m = re.search(r"remark: (.*?) \[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m or ":" not in m.group(1):
            continue
        key, value = (s.strip() for s in m.group(1).split(":", 1))
        if key == "Function Name":
            cur = out.setdefault(value, {})
        elif cur is not None:
            cur[key] = value
    return out


def text_symbols(elf):
    """{symbol name: its bytes} for the sized symbols of the ELF64 image's .text section."""
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]

    def string(table, at):
        start = sections[table][4] + at
        return elf[start:elf.index(b"\0", start)].decode()

    text = next(i for i, s in enumerate(sections) if string(shstrndx, s[0]) == ".text")
    _, _, _, text_addr, text_off, _, _, _, _, _ = sections[text]
    out = {}
    for s in sections:
        if s[1] != 2:                                   # SHT_SYMTAB
            continue
        for at in range(s[4], s[4] + s[5], s[9]):
            name, _, _, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, at)
            if shndx == text and size:
                start = text_off + value - text_addr
                out[string(s[6], name)] = elf[start:start + size]
    return out


def digest(src, csrc):
    path = src if os.path.exists(src) else os.path.join(csrc, src)
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, "device.o")
        cmd = [HIPCC] + FLAGS + ["--offload-device-only", "--no-gpu-bundle-output", "-Rpass-analysis=kernel-resource-usage",
                                 "-c", path, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(f"kernel_digest: hipcc failed on {path}:\n{r.stderr}")
        with open(obj, "rb") as f:
            symbols = text_symbols(f.read())
    report = remarks(r.stderr)
    names = sorted(report)
    demangled = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    lines = []
    for name, shown in zip(names, demangled):
        code = symbols[name]
        figures = " ".join(f"{k}={report[name].get(key)}" for k, key in REPORT)
        lines.append(f"{os.path.basename(src)} {shown} sha256={hashlib.sha256(code).hexdigest()} bytes={len(code)} {figures}")
    return sorted(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("files", nargs="+")
    ap.add_argument("--csrc", default=CSRC, help="directory that holds the translation units (default: this tree's)")
    args = ap.parse_args()
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, len(args.files))) as ex:
        for lines in ex.map(lambda s: digest(s, args.csrc), args.files):
            for line in lines:
                print(line)


if __name__ == "__main__":
    main()
