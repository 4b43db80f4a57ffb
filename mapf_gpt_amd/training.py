"""train.py's training loop (train.py:29-56 defaults, :162-165 batches, :263-276 cosine learning rate with warmup, :284-362 loop) on the
device training path of GPT (forward_backward, clip_grad_norm_, configure_optimizers -> AdamW).

    python -m mapf_gpt_amd.training --init SHAPE_OR_CKPT --data FILE_OR_DIR --val FILE_OR_DIR [--out-dir DIR] [--max-iters N] ...

--init takes a shape name ("2M", "6M", "85M", "tiny": seeded synthetic weights) or a checkpoint in the reference's layout; with --resume the
checkpoint's optimizer state, iter_num and best_val_loss are restored as train.py:190-226 does.  --data / --val are .arrow shards (or
directories of them) read through scoring.read_arrow; every file is shuffled when it is loaded, with one seeded generator, and its rows get
targets of -1 except the last position, which holds the expert action (fast_data_loader.py:39-67).  Every eval_interval iterations the
loss of eval_iters batches of each split is measured with scoring.evaluate (= estimate_loss, train.py:244-259) and a ckpt.pt is written as
train.py:298-310 writes it ({"model", "optimizer", "model_args", "iter_num", "best_val_loss", "config"}); weights.load_checkpoint and
MAPFGPTInference load it unchanged.  One JSON line per evaluation and one at the end; --log-interval N adds {"iter", "loss", "ms"} every
N iterations (train.py:346-355; 0, the default, prints none).  No GradScaler or torch.compile.

Data-parallel runs (train.py:118-138, 237-239, 314-322, 364-365): one process per GPU under torchrun,

    torchrun --standalone --nproc_per_node=N -m mapf_gpt_amd.training --init ... --data DIR --val DIR [--backend nccl|gloo]

With RANK in the environment the process joins a process group (--backend nccl = RCCL, the default, or gloo), takes cuda:LOCAL_RANK
(--share-gpu: every rank on cuda:0, for dry runs on a one-GPU box), divides gradient_accumulation_steps by the world size, reads its share of
the training split's files (fast_data_loader.py:20-28) shuffled with seed + rank, and builds the same initial weights as every other rank.
There is no DistributedDataParallel wrapper and no all_reduce: after the last micro-step of an iteration every rank exports its flat
gradient buffer, the ranks all_gather them, and one kernel adds them in rank order and scales by 1 / world (GPT.reduce_grads), so every rank
holds the same bits whatever the backend and the weights stay in lockstep without a broadcast.  param_checksum guards that: the ranks compare
it at every eval_interval boundary and at the end, and a mismatch raises on every rank.  Rank 0 alone evaluates, writes ckpt.pt and prints.
Without RANK nothing of this runs and the command behaves as a single process always did.

--rows-call runs the micro-steps through GPT.forward_backward_rows (the last layer, the head and the loss on token 255 only, no host wait;
effective dropout 0 only); --rows-call-drop runs them through GPT.forward_backward_rows_drop, the same micro-step with the general call's
dropout masks, for any --dropout or checkpoint dropout in [0, 1): the fine-tuning command is --init CKPT --dropout 0.1 --rows-call-drop.

--dtype takes train.py's knob (train.py:66-70): float32 (exact fp32, the default here) or bfloat16 (every micro-step and every estimate_loss in
the bf16 autocast regime: forward_backward(precision="bf16"), scoring.evaluate(precision="bf16")).  train.py itself defaults to bfloat16 on a
GPU that supports it; this command keeps float32 as its default.  float16 is refused: it needs a GradScaler, which this command does not have.
"""
import argparse
import glob
import json
import math
import os
import time

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


def rank_files(files, rank, world):
    """The files of `rank` among `world` data-parallel ranks, as fast_data_loader.py:20-28 deals the training split: len(files) // world
    consecutive files each, in name order; the remainder is unused.  (With more ranks than files the reference would fail on an empty list.)"""
    if not 0 <= rank < world:
        raise ValueError(f"rank {rank} outside a world of {world}")
    if world > len(files):
        raise ValueError(f"{world} ranks but only {len(files)} .arrow files: every rank needs at least one")
    per = len(files) // world
    return files[rank * per:(rank + 1) * per]


def accumulation_per_rank(gradient_accumulation_steps, world):
    """train.py:130-131: the micro-steps of an iteration are divided among the ranks."""
    if gradient_accumulation_steps % world != 0:
        raise ValueError(f"gradient_accumulation_steps = {gradient_accumulation_steps} is not a multiple of the world size {world}")
    return gradient_accumulation_steps // world


def param_checksum(net):
    """Wrap-around int64 sum of the parameters' fp32 bit patterns, computed on the device: equal on ranks whose weights are bit-identical.
    The data-parallel loop never broadcasts weights, so it compares this across the ranks instead."""
    sd = net.state_dict()
    total = torch.zeros((), dtype=torch.int64, device=net.device)
    for name, _ in net.named_parameters():
        total += sd[name].view(torch.int32).sum(dtype=torch.int64)
    return int(total.item())


class ArrowBatches:
    """= MapfArrowDataset.__iter__ (fast_data_loader.py:39-67): files in name order, forever; each file's rows shuffled when it is loaded
    (one numpy Generator seeded once), batches of batch_size consecutive rows (the last one of a file may be shorter).  Yields
    (inputs int8 [b, 256], targets int64 [b, 256]) on the host: -1 everywhere except position 255 = the expert action.  rank / world: the
    files are dealt to the ranks of a data-parallel run (rank_files) and the generator is seeded with seed + rank; the defaults change nothing.
    labels=True yields (inputs int8 [b, 256], labels int64 [b]) instead, the input of GPT.forward_backward_rows: the same generator draws
    in the same order, so labels equals the default mode's targets[:, -1] batch for batch, and no [b, 256] target matrix is built.  That
    mode validates a file's labels against [0, 67) on the host when it loads the file (ValueError), so the micro-steps need no check."""

    def __init__(self, path, batch_size, seed=1337, rank=0, world=1, labels=False):
        self.files = rank_files(shard_files(path), rank, world)
        self.batch_size = int(batch_size)
        self.labels = bool(labels)
        self.rng = np.random.Generator(np.random.PCG64(seed + rank))     # train.py:127,142: every rank its own shuffle

    def load(self, f):
        from .scoring import read_arrow
        x, y = read_arrow(f)
        idx = self.rng.permutation(len(x))
        x, y = x[idx], np.asarray(y)[idx]
        if self.labels:
            y = y.astype(np.int64)
            if len(y) and (y.min() < 0 or y.max() >= 67):
                raise ValueError(f"{f}: labels must lie in [0, 67), got [{y.min()}, {y.max()}]")
            return x, y
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


ROWS_CALL_DROPOUT = ("--rows-call with dropout {} > 0: forward_backward_rows has no dropout (its masks are not built for the compact last "
                     "layer); drop --rows-call, or pass --dropout 0")


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
    ap.add_argument("--dropout", type=float, default=None,
                    help="dropout probability of the training forward (train.py:43: 0 for pre-training, 0.1+ for fine-tuning); default: the "
                         "--init checkpoint's model_args value, 0.0 for a shape name.  Stored in the checkpoint's model_args")
    ap.add_argument("--rows-call", action="store_true",
                    help="run the micro-steps through GPT.forward_backward_rows: the last layer, head and loss on token 255 only and no "
                         "host wait per micro-step; the same gradients up to summation order.  Needs an effective dropout of 0")
    ap.add_argument("--rows-call-drop", action="store_true",
                    help="--rows-call through GPT.forward_backward_rows_drop: the same micro-step with the general call's dropout masks "
                         "(the compact last layer draws them at token 255); any effective dropout in [0, 1), 0 included")
    ap.add_argument("--log-interval", type=int, default=0,
                    help='print {"iter", "loss", "ms"} every N iterations (train.py:346-355); 0 = no such line')
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="process-group backend of a data-parallel run (RANK set): nccl = RCCL (train.py:58), gloo stages the gather through the host")
    ap.add_argument("--share-gpu", action="store_true",
                    help="data-parallel dry run on a one-GPU box: every rank uses cuda:0 instead of cuda:LOCAL_RANK")
    a = ap.parse_args(argv)
    if a.dtype == "float16":
        ap.error("--dtype float16 is not supported: it needs torch's GradScaler, which this training path does not have "
                 "(use bfloat16, which needs none, or float32)")
    if a.dropout is not None and not (0.0 <= a.dropout < 1.0):
        ap.error("--dropout must lie in [0, 1)")
    if a.rows_call and a.dropout:
        ap.error(ROWS_CALL_DROPOUT.format(a.dropout))
    if a.rows_call and a.rows_call_drop:
        ap.error("--rows-call and --rows-call-drop name two forms of one micro-step: pass one of them")
    a.precision = DTYPES[a.dtype]
    return a


def dropout_step(iter_num, total_accum, rank, world, micro):
    """The mask step of micro-step `micro` of rank `rank` in iteration `iter_num`: i * A + r * (A / world) + j with A the accumulation
    steps of the whole run.  A pure function of the loop's counters: a resumed run needs no new state, and one process that replays the
    ranks' micro-steps in rank order draws the same masks."""
    return iter_num * total_accum + rank * (total_accum // world) + micro


class Ranks:
    """The process group of a data-parallel run (train.py:118-138): RANK, LOCAL_RANK and WORLD_SIZE from the launcher's environment, the
    device cuda:LOCAL_RANK (share_gpu: cuda:0), the gradient synchronisation and the lockstep guard."""

    def __init__(self, backend, share_gpu=False):
        import torch.distributed as dist
        self.dist, self.backend = dist, backend
        self.rank, self.local_rank, world = (int(os.environ[k]) for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"))
        index = 0 if share_gpu else self.local_rank
        if index >= torch.cuda.device_count():
            raise RuntimeError(f"LOCAL_RANK {self.local_rank} but only {torch.cuda.device_count()} visible GPUs: one rank per GPU "
                               "(--share-gpu puts every rank on cuda:0 for a dry run)")
        self.device = torch.device("cuda", index)
        torch.cuda.set_device(self.device)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=self.rank, world_size=world, device_id=self.device)
        else:
            dist.init_process_group(backend, rank=self.rank, world_size=world)
        self.world = dist.get_world_size()
        self.master = self.rank == 0                   # train.py:126: evaluation, checkpoints and every stdout line
        self.coll_device = self.device if backend == "nccl" else torch.device("cpu")
        self.flat = self.gathered = None

    def sync_grads(self, net):
        """export_grads -> all_gather -> reduce_grads(gathered, 1 / world): the ranks' mean, added in rank order by one kernel, the same bits
        on every rank.  gloo has no device collectives: the buffers go through the host (as runner.gather_metrics stages its records)."""
        if self.gathered is None:
            n = net.grads_size()
            self.flat = torch.empty(n, dtype=torch.float32, device=self.device)
            self.gathered = torch.empty((self.world, n), dtype=torch.float32, device=self.device)
        net.export_grads(self.flat)
        if self.backend == "nccl":
            self.dist.all_gather_into_tensor(self.gathered, self.flat)
        else:
            host = self.flat.cpu()
            parts = [torch.empty_like(host) for _ in range(self.world)]
            self.dist.all_gather(parts, host)
            for r, part in enumerate(parts):
                self.gathered[r].copy_(part)
        net.reduce_grads(self.gathered, 1.0 / self.world)

    def check_lockstep(self, net, iter_num):
        """Every rank's param_checksum, gathered (8 bytes each); a mismatch raises on every rank.  Weights are never broadcast, so a
        divergence would otherwise be silent."""
        mine = torch.tensor([param_checksum(net)], dtype=torch.int64, device=self.coll_device)
        parts = [torch.empty_like(mine) for _ in range(self.world)]
        self.dist.all_gather(parts, mine)
        sums = [int(p.item()) for p in parts]
        if len(set(sums)) != 1:
            raise RuntimeError(f"the ranks' weights diverged at iteration {iter_num}: param_checksum per rank {sums}")
        return sums

    def close(self):
        self.dist.destroy_process_group()


def main(argv=None):
    a = parse_args(argv)
    ranks = Ranks(a.backend, a.share_gpu) if "RANK" in os.environ else None      # train.py:118: is this a data-parallel run?
    try:
        return run(a, ranks)
    finally:
        if ranks is not None:
            ranks.close()                          # train.py:364-365


def run(a, ranks):
    config = {k: getattr(a, k) for k in DEFAULTS}
    config["dtype"] = a.dtype
    from . import scoring, weights
    from .model import GPT, GPTConfig

    rank, world, master = (ranks.rank, ranks.world, ranks.master) if ranks else (0, 1, True)
    accum = accumulation_per_rank(a.gradient_accumulation_steps, world)
    ckpt = None
    if os.path.exists(a.init):
        args, sd = weights.load_checkpoint(a.init)
        if a.resume:
            ckpt = torch.load(a.init, map_location="cpu", weights_only=True)
    else:                                          # --seed on every rank: all build the weights DDP would broadcast from rank 0
        args, sd = weights.model_args(a.init), weights.synthetic_state_dict(a.init, seed=a.seed)
    if a.dropout is not None:                      # the flag overrides the checkpoint's value
        args = dict(args, dropout=float(a.dropout))
    if a.rows_call and args.get("dropout", 0.0) > 0:         # (the checkpoint's value, when no flag overrides it)
        raise SystemExit("training: " + ROWS_CALL_DROPOUT.format(args["dropout"]))
    net = GPT(GPTConfig(**args), max_rows=a.batch_size, precision="f32")
    net.load_state_dict(sd)
    net.set_dropout_rng(a.seed)                    # dropout seed = --seed; the step is set per micro-step (dropout_step)
    net.train(max_rows=a.batch_size)
    opt = net.configure_optimizers(a.weight_decay, a.learning_rate, (a.beta1, a.beta2), "cuda")
    iter_num, best_val_loss = 0, 1e9
    if ckpt is not None:
        opt.load_state_dict(ckpt["optimizer"])
        iter_num, best_val_loss = int(ckpt["iter_num"]), float(ckpt["best_val_loss"])
    train_it = iter(ArrowBatches(a.data, a.batch_size, a.seed, rank, world, labels=a.rows_call or a.rows_call_drop))     # (validated per file at load)
    val_it = iter(ArrowBatches(a.val, a.batch_size, a.seed + 1))          # (the validation split is not divided)
    if master:
        os.makedirs(a.out_dir, exist_ok=True)
    model_args = {k: args[k] for k in ("n_layer", "n_head", "n_embd", "block_size", "bias", "vocab_size", "dropout")}

    def estimate_loss():                      # train.py:244-259, eval_iters batches of each split
        out = {}
        net.eval()
        for split, it in (("train", train_it), ("val", val_it)):
            xs, ts = zip(*[next(it) for _ in range(a.eval_iters)])
            x, t = np.concatenate(xs), np.concatenate(ts)
            out[split] = scoring.evaluate(net, x, t if t.ndim == 1 else t[:, -1], batch_size=a.batch_size, precision=a.precision)["loss"]
        net.train()
        return out

    X, Y = next(train_it)
    loss = None
    t0 = time.monotonic()
    while True:
        lr = get_lr(iter_num, a.learning_rate, a.warmup_iters, a.lr_decay_iters, a.min_lr) if a.decay_lr else a.learning_rate
        for g in opt.param_groups:
            g["lr"] = lr
        if iter_num % a.eval_interval == 0 and ranks is not None:
            ranks.check_lockstep(net, iter_num)
        if iter_num % a.eval_interval == 0 and master:          # train.py:292
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
        for micro in range(accum):                             # train.py:314-331
            if a.rows_call:
                loss = net.forward_backward_rows(torch.as_tensor(X), torch.as_tensor(Y), loss_scale=1.0 / accum, precision=a.precision, check=False)
            elif a.rows_call_drop:
                loss = net.forward_backward_rows_drop(torch.as_tensor(X), torch.as_tensor(Y), loss_scale=1.0 / accum, precision=a.precision, check=False,
                                                      dropout_step=dropout_step(iter_num, a.gradient_accumulation_steps, rank, world, micro))
            else:
                loss = net.forward_backward(torch.as_tensor(X), torch.as_tensor(Y), loss_scale=1.0 / accum, precision=a.precision,
                                            dropout_step=dropout_step(iter_num, a.gradient_accumulation_steps, rank, world, micro))
            X, Y = next(train_it)
        if ranks is not None:                                  # train.py:315-322: the ranks' gradients meet after the last micro-step
            ranks.sync_grads(net)
        if a.grad_clip != 0.0:
            net.clip_grad_norm_(a.grad_clip)
        opt.step()
        opt.zero_grad(set_to_none=True)
        if a.log_interval > 0 and iter_num % a.log_interval == 0 and master:      # train.py:346-355 (float(loss) waits for the device)
            lossf, t1 = float(loss), time.monotonic()
            print(json.dumps({"iter": iter_num, "loss": lossf, "ms": round((t1 - t0) * 1e3, 3)}), flush=True)
        t0 = time.monotonic()
        iter_num += 1
        if iter_num > a.max_iters:
            break
    res = {"iter": iter_num, "loss": float(loss), "best_val_loss": float(best_val_loss)}
    if ranks is not None:
        res["world"] = world
        res["param_checksums"] = ranks.check_lockstep(net, iter_num)
    if master:
        print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main()
