"""python -m mapf_gpt_amd.training --rows-call-drop --dropout P under RANK / WORLD_SIZE, in the manner of
tests/test_gpu_train_dropout_ddp.py (whose shards, command line and child-process runner come from tests/test_gpu_train_ddp.py): two ranks
over gloo sharing the GPU end, bit for bit, with the checkpoint of one process that replays their micro-steps in rank order through
GPT.forward_backward_rows_drop at the mask steps of training.dropout_step.  The rows call sees the same gradient buffer as the general one,
so sync_grads is untouched; this is also the first data-parallel run of the last-position micro-step."""
import numpy as np
import pytest
import torch

from mapf_gpt_amd import training, weights
from mapf_gpt_amd.model import GPT, GPTConfig
from tests.test_gpu_train_ddp import ACCUM, BATCH, EVAL_INTERVAL, EVAL_ITERS, SCHEDULE, SEED, _bits, _two_ranks
from tests.test_gpu_train_ddp import data      # noqa: F401  (the module-scoped shard fixture)
from tests.test_gpu_train_dropout_ddp import P, _same_weights

pytestmark = pytest.mark.gpu


def _replay_rows(data, world, max_iters, precision, drop=True):
    """The run of `world` ranks in one process: per iteration each rank's micro-steps on (rows, labels) from its own iterator at the steps of
    training.dropout_step, the rank-ordered mean, clip, AdamW.  The master's estimate_loss draws eval_iters training batches at every
    eval_interval boundary after the loop's first batch was fetched; they are drawn here too.  drop=False: the dropout-free rows call.
    -> (net, {iteration: state_dict at that boundary})"""
    args, sd = dict(weights.model_args("tiny"), dropout=P if drop else 0.0), weights.synthetic_state_dict("tiny", seed=SEED)
    net = GPT(GPTConfig(**args), max_rows=BATCH, precision="f32")
    net.load_state_dict(sd)
    net.set_dropout_rng(SEED)
    net.train(max_rows=BATCH)
    opt = net.configure_optimizers(training.DEFAULTS["weight_decay"], SCHEDULE["learning_rate"],
                                   (training.DEFAULTS["beta1"], training.DEFAULTS["beta2"]))
    its = [iter(training.ArrowBatches(str(data / "train"), BATCH, SEED, r, world, labels=True)) for r in range(world)]
    cur = [next(it) for it in its]
    gathered = torch.empty((world, net.grads_size()), dtype=torch.float32, device="cuda")
    per_rank = ACCUM // world
    saved = {}
    for iter_num in range(max_iters + 1):
        lr = training.get_lr(iter_num, **SCHEDULE)
        for g in opt.param_groups:
            g["lr"] = lr
        if iter_num % EVAL_INTERVAL == 0:
            saved[iter_num] = {k: v.cpu() for k, v in net.state_dict().items()}
            for _ in range(EVAL_ITERS):
                next(its[0])
        for r in range(world):
            net.zero_grad()
            for j in range(per_rank):
                net.forward_backward_rows_drop(torch.as_tensor(cur[r][0]), torch.as_tensor(cur[r][1]), loss_scale=1.0 / per_rank, precision=precision,
                                               check=False, dropout_step=training.dropout_step(iter_num, ACCUM, r, world, j))
                cur[r] = next(its[r])
            net.export_grads(gathered[r])
        net.reduce_grads(gathered, 1.0 / world)
        net.clip_grad_norm_(training.DEFAULTS["grad_clip"])
        opt.step()
        opt.zero_grad(set_to_none=True)
    return net, saved


@pytest.mark.parametrize("dtype,precision,port", [("float32", "f32", 29591), ("bfloat16", "bf16", 29597)])
def test_two_ranks_rows_call_drop_equal_one_process(data, tmp_path, dtype, precision, port):
    lines, ckpt = _two_ranks(data, tmp_path, port, "--rows-call-drop", "--dropout", str(P), "--dtype", dtype, "--max-iters", "3")
    net, saved = _replay_rows(data, 2, 3, precision)
    assert training.param_checksum(net) == lines[-1]["param_checksums"][0]
    raw = torch.load(ckpt, map_location="cpu", weights_only=True)
    assert raw["iter_num"] == 2 and raw["model_args"]["dropout"] == P
    _same_weights(raw, saved[2])
    # ... and dropout did something: the dropout-free replay of the same micro-steps ends elsewhere
    plain, _ = _replay_rows(data, 2, 3, precision, drop=False)
    assert training.param_checksum(plain) != lines[-1]["param_checksums"][0]
    assert not all(np.array_equal(_bits(v), _bits(plain.state_dict()[k].cpu())) for k, v in raw["model"].items())
