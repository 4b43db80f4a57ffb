"""Validation loss and greedy-action accuracy of a checkpoint on expert data (= train.py:244-257 estimate_loss over a whole split).

The dataset rows are 256 int8 tokens with targets -1 everywhere but position 255, which holds the expert's action
(dataset/fast_data_loader.py:34,58).  So the reference's F.cross_entropy(ignore_index=-1) of a batch is the mean over its rows of
-log softmax(logits of position 255)[action]: `GPT.score_tokens` computes that per row from the same forward as act_tokens, and the
hit flag compares the action with the greedy choice of act(do_sample=False).

    python -m mapf_gpt_amd.scoring --weights CKPT --data FILE_OR_DIR [--precision f32|f16x3|bf16] [--batch-size N]

prints one JSON line {loss, accuracy, rows, effective_precision, rows_per_s}.  Inputs may also come from
dataset_tokenizer.ObservationGenerator.generate_observations (its (inputs, gt_actions) plug straight into `evaluate`).
"""
import argparse
import glob
import json
import os
import time

import numpy as np
import torch


def _effective_precision(net, precision):
    p = precision or net.precision
    p = "f32" if p == "fp32" else p
    if p == "f16x3":
        return net.envelope()["effective_precision"]
    return p


@torch.no_grad()
def evaluate(net, inputs, gt_actions, batch_size=4096, precision=None):
    """inputs [N, 256] int8 / uint8 token rows (numpy or torch, host or device), gt_actions [N] -> {"loss": mean NLL of the expert actions,
    "accuracy": fraction of rows whose greedy action is the expert's, "rows": N, "effective_precision": the kernels that ran}."""
    inputs = torch.as_tensor(inputs)
    gt = torch.as_tensor(gt_actions).reshape(-1)
    if inputs.dim() != 2 or inputs.shape[1] != 256:
        raise ValueError(f"inputs must be [N, 256] token rows, got {tuple(inputs.shape)}")
    n = inputs.shape[0]
    if gt.numel() != n:
        raise ValueError(f"{n} rows but {gt.numel()} actions")
    nll_sum = torch.zeros((), dtype=torch.float64, device=net.device)
    hits = torch.zeros((), dtype=torch.int64, device=net.device)
    for r0 in range(0, n, batch_size):
        tok = inputs[r0:r0 + batch_size].to(device=net.device).to(torch.uint8).contiguous()   # (int8 ids 0 .. 66: same bits)
        nll, hit = net.score_tokens(tok, gt[r0:r0 + batch_size], precision=precision)
        nll_sum += nll.double().sum()
        hits += hit.sum()
    return {"loss": float(nll_sum) / n if n else float("nan"), "accuracy": int(hits) / n if n else float("nan"), "rows": int(n),
            "effective_precision": _effective_precision(net, precision)}


def read_arrow(path_or_dir):
    """Expert data in the reference's shard format (fast_data_loader.py:39-50: Arrow IPC files with columns input_tensors and gt_actions,
    memory-mapped) -> (inputs int8 [N, 256], gt_actions [N]).  A directory reads its *.arrow files in name order; rows keep file order
    (no shuffle).  Needs pyarrow."""
    try:
        import pyarrow as pa
    except ImportError as e:     # optional dependency: only this reader needs it
        raise ImportError("mapf_gpt_amd.scoring.read_arrow needs pyarrow (pip install pyarrow)") from e
    files = sorted(glob.glob(os.path.join(path_or_dir, "*.arrow"))) if os.path.isdir(path_or_dir) else [path_or_dir]
    if not files:
        raise FileNotFoundError(f"no .arrow files in {path_or_dir}")
    xs, ys = [], []
    for f in files:
        with pa.memory_map(f) as source:
            table = pa.ipc.open_file(source).read_all()
            x = table["input_tensors"].to_numpy(zero_copy_only=False)
            y = table["gt_actions"].to_numpy(zero_copy_only=False)
        xs.append(np.stack(x).astype(np.int8) if len(x) else np.zeros((0, 256), np.int8))
        ys.append(np.asarray(y))
    return np.concatenate(xs), np.concatenate(ys)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--weights", required=True, help="checkpoint in the reference's layout ({'model': state_dict, 'model_args': {...}})")
    ap.add_argument("--data", required=True, help=".arrow shard or a directory of them")
    ap.add_argument("--precision", default="f16x3", choices=["f32", "f16x3", "bf16"])
    ap.add_argument("--batch-size", type=int, default=4096)
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    from . import weights
    from .model import GPT, GPTConfig
    args, sd = weights.load_checkpoint(a.weights)
    net = GPT(GPTConfig(**args), max_rows=a.batch_size, precision=a.precision, device=a.device)
    net.load_state_dict(sd)
    inputs, gt = read_arrow(a.data)
    t0 = time.perf_counter()
    res = evaluate(net, inputs, gt, batch_size=a.batch_size)
    torch.cuda.synchronize(net.device)
    dt = time.perf_counter() - t0
    res["rows_per_s"] = res["rows"] / dt if dt > 0 else None
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
