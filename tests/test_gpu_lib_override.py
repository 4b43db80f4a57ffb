"""MGPT_LIB_PATH on the device: a byte copy of the installed library, loaded by path in a fresh process, computes the same bits."""
import os
import shutil
import subprocess
import sys

import pytest

from mapf_gpt_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = """
import hashlib
import numpy as np
import torch
from mapf_gpt_amd.model import build_model
net = build_model("tiny", seed=3, envelope="ignore", max_rows=4)
tokens = torch.from_numpy(np.random.default_rng(5).integers(0, 67, size=(3, 256), dtype=np.uint8)).cuda()
logits = net.logits_tokens(tokens, precision="f16x3")
torch.cuda.synchronize()
print("digest", hashlib.sha256(logits.cpu().contiguous().numpy().tobytes()).hexdigest())
"""


@pytest.mark.gpu
def test_copy_loaded_by_path_computes_the_same_bits(tmp_path):
    copy = str(tmp_path / "lib_copy.so")
    shutil.copyfile(build.build(), copy)
    digests = []
    for lib_path in (None, copy):
        env = {k: v for k, v in os.environ.items() if k != "MGPT_LIB_PATH"}
        if lib_path is not None:
            env["MGPT_LIB_PATH"] = lib_path
        r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        said = f"mapf_gpt_amd: library from MGPT_LIB_PATH={copy}" in r.stderr
        assert said == (lib_path is not None), r.stderr[-2000:]
        digests.append(next(line.split()[1] for line in r.stdout.splitlines() if line.startswith("digest ")))
    assert len(digests[0]) == 64 and digests[0] == digests[1]
