"""train.py's training loop (train.py:29-56 defaults, :162-165 batches, :263-276 cosine learning rate with warmup, :284-362 loop) on the
device training path of GPT (forward_backward, clip_grad_norm_, configure_optimizers -> AdamW).

    python -m mapf_gpt_amd.training --init SHAPE_OR_CKPT --data FILE_OR_DIR --val FILE_OR_DIR [--out-dir DIR] [--max-iters N] ...

--init takes a shape name ("2M", "6M", "85M", "tiny": seeded synthetic weights) or a checkpoint in the reference's layout; with --resume the
checkpoint's optimizer state, iter_num and best_val_loss are restored as train.py:190-226 does.  --data / --val are .arrow shards (or
directories of them) read through scoring.read_arrow; every file is shuffled when it is loaded, with one seeded generator, and its rows get
targets of -1 except the last position, which holds the expert action (fast_data_loader.py:39-67).  Every eval_interval iterations the
loss of eval_iters batches of each split is measured with scoring.evaluate (= estimate_loss, train.py:244-259) and a ckpt.pt is written as
train.py:298-310 writes it ({"model", "optimizer", "model_args", "iter_num", "best_val_loss", "config"}); weights.load_checkpoint and
MAPFGPTInference load it unchanged.  One JSON line per evaluation and one at the end.  No DDP, GradScaler or torch.compile.

--dtype takes train.py's knob (train.py:66-70): float32 (exact fp32, the default here) or bfloat16 (every micro-step and every estimate_loss in
the bf16 autocast regime: forward_backward(precision="bf16"), scoring.evaluate(precision="bf16")).  train.py itself defaults to bfloat16 on a
GPU that supports it; this command keeps float32 as its default.  float16 is refused: it needs a GradScaler, which this command does not have.
"""
import argparse
import glob
import json
import math
import os

import numpy as np
import torch

DEFAULTS = dict(              # train.py:29-56
    eval_interval=500, eval_iters=40, always_save_checkpoint=True, gradient_accumulation_steps=16, batch_size=64,
    learning_rate=6e-4, max_iters=30000, weight_decay=1e-1, beta1=0.9, beta2=0.95, grad_clip=1.0, decay_lr=True,
    warmup_iters=2000, lr_decay_iters=30000, min_lr=6e-5,
)


def get_lr(it, learning_rate, warmup_iters, lr_decay_iters, min_lr):
    """train.py:263-274: linear warmup, cosine decay to min_lr, then min_lr."""
    if it < warmup_iters:
        return learning_rate * it / warmup_iters
    if it > lr_decay_iters:
        return min_lr
    decay_ratio = (it - warmup_iters) / (lr_decay_iters - warmup_iters)
    assert 0 <= decay_ratio <= 1
    coeff = 0.5 * (1.0 + math.cos(math.pi * decay_ratio))
    return min_lr + coeff * (learning_rate - min_lr)


def shard_files(path):
    files = sorted(glob.glob(os.path.join(path, "*.arrow"))) if os.path.isdir(path) else [path]
    if not files:
        raise FileNotFoundError(f"no .arrow files in {path}")
    return files


class ArrowBatches:
    """= MapfArrowDataset.__iter__ (fast_data_loader.py:39-67): files in name order, forever; each file's rows shuffled when it is loaded
    (one numpy Generator seeded once), batches of batch_size consecutive rows (the last one of a file may be shorter).  Yields
    (inputs int8 [b, 256], targets int64 [b, 256]) on the host: -1 everywhere except position 255 = the expert action."""

    def __init__(self, path, batch_size, seed=1337):
        self.files = shard_files(path)
        self.batch_size = int(batch_size)
        self.rng = np.random.Generator(np.random.PCG64(seed))

    def load(self, f):
        from .scoring import read_arrow
        x, y = read_arrow(f)
        idx = self.rng.permutation(len(x))
        x, y = x[idx], np.asarray(y)[idx]
        t = np.full(x.shape, -1, np.int64)
        t[:, -1] = y
        return x, t

    def __iter__(self):
        while True:
            for f in self.files:
                x, t = self.load(f)
                for i in range(0, len(x), self.batch_size):
                    yield x[i:i + self.batch_size], t[i:i + self.batch_size]


def _cpu(obj):
    if torch.is_tensor(obj):
        return obj.detach().cpu()
    if isinstance(obj, dict):
        return {k: _cpu(v) for k, v in obj.items()}
    if isinstance(obj, list):
        return [_cpu(v) for v in obj]
    return obj


DTYPES = {"float32": "f32", "bfloat16": "bf16"}       # --dtype (train.py:66-70) -> precision of forward_backward and scoring.evaluate


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--init", required=True, help='shape name ("2M", "6M", "85M", "tiny") or a checkpoint path')
    ap.add_argument("--resume", action="store_true", help="restore optimizer state, iter_num and best_val_loss from the --init checkpoint")
    ap.add_argument("--data", required=True, help="training .arrow shard or directory")
    ap.add_argument("--val", required=True, help="validation .arrow shard or directory")
    ap.add_argument("--out-dir", default="out")
    ap.add_argument("--seed", type=int, default=1337, help="initial weights of a shape name, and the shuffle")
    for k, v in DEFAULTS.items():
        if isinstance(v, bool):
            ap.add_argument("--" + k.replace("_", "-"), type=lambda s: s.lower() in ("1", "true", "yes"), default=v)
        else:
            ap.add_argument("--" + k.replace("_", "-"), type=type(v), default=v)
    ap.add_argument("--dtype", default="float32", choices=["float32", "bfloat16", "float16"],
                    help="float32 (default here; train.py defaults to bfloat16) or bfloat16 (autocast regime); float16 is refused")
    a = ap.parse_args(argv)
    if a.dtype == "float16":
        ap.error("--dtype float16 is not supported: it needs torch's GradScaler, which this training path does not have "
                 "(use bfloat16, which needs none, or float32)")
    a.precision = DTYPES[a.dtype]
    return a


def main(argv=None):
    a = parse_args(argv)
    config = {k: getattr(a, k) for k in DEFAULTS}
    config["dtype"] = a.dtype
    from . import scoring, weights
    from .model import GPT, GPTConfig

    ckpt = None
    if os.path.exists(a.init):
        args, sd = weights.load_checkpoint(a.init)
        if a.resume:
            ckpt = torch.load(a.init, map_location="cpu", weights_only=True)
    else:
        args, sd = weights.model_args(a.init), weights.synthetic_state_dict(a.init, seed=a.seed)
    net = GPT(GPTConfig(**args), max_rows=a.batch_size, precision="f32")
    net.load_state_dict(sd)
    net.train(max_rows=a.batch_size)
    opt = net.configure_optimizers(a.weight_decay, a.learning_rate, (a.beta1, a.beta2), "cuda")
    iter_num, best_val_loss = 0, 1e9
    if ckpt is not None:
        opt.load_state_dict(ckpt["optimizer"])
        iter_num, best_val_loss = int(ckpt["iter_num"]), float(ckpt["best_val_loss"])
    train_it = iter(ArrowBatches(a.data, a.batch_size, a.seed))
    val_it = iter(ArrowBatches(a.val, a.batch_size, a.seed + 1))
    os.makedirs(a.out_dir, exist_ok=True)
    model_args = {k: args[k] for k in ("n_layer", "n_head", "n_embd", "block_size", "bias", "vocab_size", "dropout")}

    def estimate_loss():                      # train.py:244-259, eval_iters batches of each split
        out = {}
        net.eval()
        for split, it in (("train", train_it), ("val", val_it)):
            xs, ts = zip(*[next(it) for _ in range(a.eval_iters)])
            x, t = np.concatenate(xs), np.concatenate(ts)
            out[split] = scoring.evaluate(net, x, t[:, -1], batch_size=a.batch_size, precision=a.precision)["loss"]
        net.train()
        return out

    X, Y = next(train_it)
    loss = None
    while True:
        lr = get_lr(iter_num, a.learning_rate, a.warmup_iters, a.lr_decay_iters, a.min_lr) if a.decay_lr else a.learning_rate
        for g in opt.param_groups:
            g["lr"] = lr
        if iter_num % a.eval_interval == 0:
            losses = estimate_loss()
            rec = {"iter": iter_num, "train_loss": losses["train"], "val_loss": losses["val"], "lr": lr}
            if losses["val"] < best_val_loss or a.always_save_checkpoint:
                best_val_loss = losses["val"]
                if iter_num > 0:
                    torch.save({"model": _cpu(net.state_dict()), "optimizer": _cpu(opt.state_dict()), "model_args": model_args,
                                "iter_num": iter_num, "best_val_loss": best_val_loss, "config": config},
                               os.path.join(a.out_dir, "ckpt.pt"))
                    rec["saved"] = os.path.join(a.out_dir, "ckpt.pt")
            print(json.dumps(rec), flush=True)
        for _ in range(a.gradient_accumulation_steps):         # train.py:314-331
            loss = net.forward_backward(torch.as_tensor(X), torch.as_tensor(Y), loss_scale=1.0 / a.gradient_accumulation_steps,
                                       precision=a.precision)
            X, Y = next(train_it)
        if a.grad_clip != 0.0:
            net.clip_grad_norm_(a.grad_clip)
        opt.step()
        opt.zero_grad(set_to_none=True)
        iter_num += 1
        if iter_num > a.max_iters:
            break
    res = {"iter": iter_num, "loss": float(loss), "best_val_loss": float(best_val_loss)}
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main()
