"""CPU checks of the evaluation feature (GPT.forward(idx, targets), mapf_gpt_amd/scoring.py): the tests' own restatement of
model.py:178-184 against goldens of the real reference, and the .arrow reader."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mapf_gpt_amd import weights
from oracle import gpt_oracle
from tests.helpers import GOLDEN


def seq_oracle(sd, args, tokens, targets=None, dtype=torch.float32):
    """model.py:178-184 on the pinned oracle's residual after the last block: ln_f, @ wte^T at every position, cross-entropy (ignore_index=-1)."""
    x = gpt_oracle.forward_logits(sd, args, tokens, dtype=dtype, return_layers=True)[1][-1]
    w = gpt_oracle.to_torch(sd, dtype)
    h = F.layer_norm(x, (x.shape[-1],), w["transformer.ln_f.weight"], w.get("transformer.ln_f.bias"), 1e-5)
    logits = h @ w["lm_head.weight"].t()
    loss = None
    if targets is not None:
        loss = F.cross_entropy(logits.reshape(-1, 67), torch.as_tensor(targets).long().reshape(-1), ignore_index=-1)
    return logits, loss


@pytest.mark.parametrize("name", ["tiny", "6M"])
def test_head_restatement_matches_reference_golden(name):
    g = np.load(os.path.join(GOLDEN, f"loss_{name}.npz"))
    sd = weights.synthetic_state_dict(name, seed=int(g["seed"]), scale=float(g["scale"]))
    logits, loss = seq_oracle(sd, weights.model_args(name), g["tokens"], g["targets"])
    got = logits[:, g["positions"], :].numpy()
    assert np.abs(got - g["logits"]).max() <= 1e-5
    assert abs(float(loss) - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    # the golden's row patterns: every position, position 255 only, none, about half
    t = g["targets"]
    assert (t[0] >= 0).all() and (t[1, :255] == -1).all() and t[1, 255] >= 0 and (t[2] == -1).all() and 0 < (t[3] >= 0).sum() < 256


def test_read_arrow_round_trip(tmp_path):
    pa = pytest.importorskip("pyarrow")
    from mapf_gpt_amd import scoring
    rng = np.random.Generator(np.random.PCG64(2))
    shards = []
    for k, n in enumerate((5, 3)):
        x = rng.integers(0, 67, (n, 256)).astype(np.int8)
        y = rng.integers(0, 5, n).astype(np.int8)
        # the reference's shard layout (fast_data_loader.py:39-50): one list column of token rows, one column of actions
        table = pa.table({"input_tensors": pa.array(list(x)), "gt_actions": pa.array(y)})
        with pa.OSFile(str(tmp_path / f"part_{k}.arrow"), "wb") as sink:
            with pa.ipc.new_file(sink, table.schema) as w:
                w.write_table(table)
        shards.append((x, y))
    x1, y1 = scoring.read_arrow(str(tmp_path / "part_1.arrow"))
    assert x1.dtype == np.int8 and x1.shape == (3, 256) and np.array_equal(x1, shards[1][0]) and np.array_equal(y1, shards[1][1])
    xa, ya = scoring.read_arrow(str(tmp_path))          # a directory: files in name order, rows in file order
    assert np.array_equal(xa, np.concatenate([s[0] for s in shards])) and np.array_equal(ya, np.concatenate([s[1] for s in shards]))


def test_evaluate_rejects_bad_shapes():
    from mapf_gpt_amd import scoring
    with pytest.raises(ValueError):
        scoring.evaluate(None, np.zeros((4, 255), np.int8), np.zeros(4, np.int8))
    with pytest.raises(ValueError):
        scoring.evaluate(None, np.zeros((4, 256), np.int8), np.zeros(3, np.int8))
