"""python -m mapf_gpt_amd.training --dropout P, alone and under RANK / WORLD_SIZE (in the manner of tests/test_gpu_train_ddp.py, whose
shards, command line and child-process runner are used here): the value lands in the checkpoint's model_args, and the runs end, bit for bit,
with the weights of one process that replays their micro-steps from the public pieces with the mask step of training.dropout_step --
i * A + r * (A / world) + j, a function of the loop's counters alone, so a resumed run needs no state beyond iter_num."""
import numpy as np
import pytest
import torch

from mapf_gpt_amd import training, weights
from mapf_gpt_amd.model import GPT, GPTConfig
from tests.test_gpu_train_ddp import ACCUM, BATCH, EVAL_INTERVAL, EVAL_ITERS, SCHEDULE, SEED, _bits, _command, _plain_env, _run_all, _two_ranks
from tests.test_gpu_train_ddp import data      # noqa: F401  (the module-scoped shard fixture)

pytestmark = pytest.mark.gpu

P = 0.1


def _replay(data, world, max_iters, precision, ckpt=None):
    """The run of `world` ranks in one process: per iteration each rank's micro-steps from its own iterator at the steps of
    training.dropout_step, the rank-ordered mean (world > 1), clip, AdamW.  ckpt: continue from that checkpoint as --resume does (weights,
    optimizer state, iter_num; fresh iterators).  The master's estimate_loss draws eval_iters training batches at every eval_interval
    boundary after the loop's first batch was fetched; they are drawn here too.  -> (net, {iteration: state_dict at that boundary})"""
    args, sd, start = dict(weights.model_args("tiny"), dropout=P), weights.synthetic_state_dict("tiny", seed=SEED), 0
    if ckpt is not None:
        args, sd = weights.load_checkpoint(str(ckpt))
        assert args["dropout"] == P
    net = GPT(GPTConfig(**args), max_rows=BATCH, precision="f32")
    net.load_state_dict(sd)
    net.set_dropout_rng(SEED)
    net.train(max_rows=BATCH)
    opt = net.configure_optimizers(training.DEFAULTS["weight_decay"], SCHEDULE["learning_rate"],
                                   (training.DEFAULTS["beta1"], training.DEFAULTS["beta2"]))
    if ckpt is not None:
        raw = torch.load(ckpt, map_location="cpu", weights_only=True)
        opt.load_state_dict(raw["optimizer"])
        start = int(raw["iter_num"])
    its = [iter(training.ArrowBatches(str(data / "train"), BATCH, SEED, r, world)) for r in range(world)]
    cur = [next(it) for it in its]
    gathered = torch.empty((world, net.grads_size()), dtype=torch.float32, device="cuda")
    per_rank = ACCUM // world
    saved = {}
    for iter_num in range(start, max_iters + 1):
        lr = training.get_lr(iter_num, **SCHEDULE)
        for g in opt.param_groups:
            g["lr"] = lr
        if iter_num % EVAL_INTERVAL == 0:
            saved[iter_num] = {k: v.cpu() for k, v in net.state_dict().items()}
            for _ in range(EVAL_ITERS):
                next(its[0])
        for r in range(world):
            if world > 1:
                net.zero_grad()
            for j in range(per_rank):
                net.forward_backward(torch.as_tensor(cur[r][0]), torch.as_tensor(cur[r][1]), loss_scale=1.0 / per_rank, precision=precision,
                                     dropout_step=training.dropout_step(iter_num, ACCUM, r, world, j))
                cur[r] = next(its[r])
            if world > 1:
                net.export_grads(gathered[r])
        if world > 1:
            net.reduce_grads(gathered, 1.0 / world)
        net.clip_grad_norm_(training.DEFAULTS["grad_clip"])
        opt.step()
        opt.zero_grad(set_to_none=True)
    return net, saved


def _same_weights(raw, want):
    assert set(raw["model"]) == set(want)
    for k, v in raw["model"].items():
        assert np.array_equal(_bits(v), _bits(want[k])), k


def test_cli_dropout_lands_in_the_checkpoint_and_resumes(data, tmp_path):
    """--init tiny --dropout 0.1 writes model_args["dropout"] = 0.1 and the weights of the replay.  A run resumed from that checkpoint without
    the flag takes the checkpoint's 0.1 and ends, bit for bit, with the weights of the replay that continues from the same checkpoint: the
    masks of iteration i are those of step i * A + j whether or not the process was restarted in between.  (The shuffle of a resumed run
    starts over, as the reference's loader does, so its batches are not those an uninterrupted run would have drawn; the replay starts its
    iterator over in the same way.)"""
    def run(out, *extra):
        (lines,), _ = _run_all([(_command(data, tmp_path / out, "--always-save-checkpoint", "true", *extra), _plain_env())], 600)
        return lines, torch.load(tmp_path / out / "ckpt.pt", map_location="cpu", weights_only=True)

    lines, raw = run("first", "--dropout", str(P), "--max-iters", "3")
    assert raw["model_args"]["dropout"] == P and raw["iter_num"] == 2 and lines[-1]["iter"] == 4
    _, saved = _replay(data, 1, 2, "f32")
    _same_weights(raw, saved[2])
    lines, again = run("second", "--init", str(tmp_path / "first" / "ckpt.pt"), "--resume", "--max-iters", "4")
    assert again["model_args"]["dropout"] == P and again["iter_num"] == 4 and lines[-1]["iter"] == 5
    _, saved = _replay(data, 1, 4, "f32", ckpt=tmp_path / "first" / "ckpt.pt")
    _same_weights(again, saved[4])
    assert not all(np.array_equal(_bits(again["model"][k]), _bits(raw["model"][k])) for k in raw["model"])


@pytest.mark.parametrize("dtype,precision,port", [("float32", "f32", 29581), ("bfloat16", "bf16", 29587)])
def test_two_ranks_with_dropout_equal_one_process(data, tmp_path, dtype, precision, port):
    lines, ckpt = _two_ranks(data, tmp_path, port, "--dropout", str(P), "--dtype", dtype, "--max-iters", "3")
    net, saved = _replay(data, 2, 3, precision)
    assert training.param_checksum(net) == lines[-1]["param_checksums"][0]
    raw = torch.load(ckpt, map_location="cpu", weights_only=True)
    assert raw["iter_num"] == 2 and raw["model_args"]["dropout"] == P
    _same_weights(raw, saved[2])
    # ... and dropout did something: the dropout-free replay of tests/test_gpu_train_ddp.py ends elsewhere
    from tests.test_gpu_train_ddp import _replay as plain_replay
    assert training.param_checksum(plain_replay(data, 3, precision)[0]) != lines[-1]["param_checksums"][0]
