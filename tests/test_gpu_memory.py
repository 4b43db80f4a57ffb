"""Every context gives back exactly the device memory it took (mgpt_mem_debug: live allocations and bytes of the library's arenas,
csrc/device_mem.h).  Each item is built, used once and destroyed twice: the counters return to where they were (exact equality), and the
second build holds exactly the bytes of the first -- a buffer allocated twice, dropped or left behind shows in one or the other."""
import gc

import numpy as np
import pytest
import torch

from mapf_gpt_amd import _lib, weights

pytestmark = pytest.mark.gpu


def live():
    torch.cuda.synchronize()
    gc.collect()
    return _lib.mem_debug()


# one shape per builder of gpt_fast.hip's ModeBuilder, n_layer = 2 (the layer-0 table of the 6M family needs L > 1)
GPT_SHAPES = {
    "register_c64": dict(n_layer=2, n_head=2, n_embd=64),
    "register_c160": dict(n_layer=2, n_head=5, n_embd=160),      # with the 160-only persistent streams
    "6m_c256_h8": dict(n_layer=2, n_head=8, n_embd=256),
    "packed_c256_h4": dict(n_layer=2, n_head=4, n_embd=256),     # bf16 also takes the LayerNorm-fold packings
}


def gpt_cycle(args):
    """build, forward in both 16-bit modes, a one-row forward (the lazy head_parts where the plan is head-parallel), reload and forward
    again (free_mode + rebuild) -> the counters with the model built; the model is destroyed on return"""
    from mapf_gpt_amd.model import GPT, GPTConfig
    sd = weights.synthetic_state_dict(args, seed=3)
    net = GPT(GPTConfig(**weights.model_args(args)), max_rows=2, precision="f16x3")
    net.load_state_dict(sd)
    tok = torch.from_numpy(np.random.default_rng(0).integers(0, 67, (2, 256), dtype=np.uint8)).cuda()
    for prec in ("f16x3", "bf16"):
        assert torch.isfinite(net.logits_tokens(tok, precision=prec)).all()
    assert torch.isfinite(net.logits_tokens(tok[:1], precision="f16x3")).all()
    net.load_state_dict(sd)
    assert torch.isfinite(net.logits_tokens(tok, precision="f16x3")).all()
    built = live()
    del net
    return built


@pytest.mark.parametrize("shape", sorted(GPT_SHAPES))
def test_gpt_modes_give_back_what_they_took(shape):
    before = live()
    built = []
    for _ in range(2):
        built.append(gpt_cycle(GPT_SHAPES[shape]))
        assert built[-1][0] > before[0] and built[-1][1] > before[1]
        assert live() == before
    assert built[0] == built[1]


def small_world():
    from mapf_gpt_amd.runner import make_instances
    grid = np.zeros((20, 20), np.uint8)
    grid[5, 3:12] = 1
    grid[12, 8:17] = 1
    pos, goal = make_instances(grid, 2, 4, first_seed=0)
    return grid, pos, goal


def runner_cycle():
    """tokenizer + env + step on the tiny model; retire switched on and off; lifelong queues set and cleared"""
    from mapf_gpt_amd.model import build_model
    from mapf_gpt_amd.runner import BatchedRunner
    grid, pos, goal = small_world()
    net = build_model("tiny", max_rows=8, precision="f16x3")
    run = BatchedRunner(grid, 2, 4, net, max_episode_steps=16, seed=1)
    run.reset(pos, goal)
    run.run(2)
    for on in (True, False, True):
        run.set_retire_done(on)
        run.reset(pos, goal)
        run.run(2)
    built = live()
    run.set_retire_done(False)
    plain = live()
    assert plain[0] == built[0] - 5 and plain[1] < built[1]        # live list, its count (device + pinned), compact tokens and logits
    queue = goal[:, :, None, :].repeat(1, 1, 3, 1).contiguous()    # int16 [2, 4, 3, 2]
    for _ in range(2):                                             # the second call replaces the queues of the first
        run.env.set_lifelong(queue)
        assert live() == (plain[0] + 3, plain[1] + queue.numel() * 2 + 2 * (2 * 4) * 4)
    run.env.set_lifelong(None)
    assert live() == plain
    del run, net
    return built


def expert_cycle():
    """expert with the LaCAM search and the swap rule; set_swap off and on again (the degree map is built once)"""
    from mapf_gpt_amd.expert import BatchedExpert
    grid, pos, goal = small_world()
    ex = BatchedExpert(grid, 2, 4, 16, seed=1, search="lacam", max_iters=8, swap=True)
    with_map = live()
    ex.set_swap(False)
    ex.set_swap(True)
    assert live() == with_map
    ex.reset(pos, goal)
    ex.run(4)
    built = live()
    assert built == with_map
    del ex
    return built


def dedup_cycle():
    from mapf_gpt_amd.dataset_build import DedupSet
    ds = DedupSet(64)
    rows = torch.from_numpy(np.random.default_rng(1).integers(0, 67, (64, 256), dtype=np.uint8)).to(ds.device)
    assert int(ds.filter(rows[:32]).sum()) == 32 and int(ds.filter(rows[16:48]).sum()) == 16      # (64 rows offered: the capacity)
    built = live()
    del ds
    return built


def train_cycle():
    """train_alloc(1), train_alloc(2) (the activation part is re-sized, the optimizer state stays), train_free"""
    from mapf_gpt_amd.model import build_model
    net = build_model("tiny", max_rows=2, precision="f32")
    model_only = live()
    idx = torch.from_numpy(np.random.default_rng(2).integers(0, 67, (2, 256), dtype=np.int64)).cuda()
    net.train(max_rows=1)
    one_row = live()
    assert torch.isfinite(net.forward_backward(idx, idx))
    net.train(max_rows=2)
    built = live()
    assert built[0] == one_row[0] and built[1] > one_row[1]
    assert torch.isfinite(net.forward_backward(idx, idx, precision="bf16"))
    _lib.check(_lib.lib().mgpt_gpt_train_free(net._h))
    net._train_rows = None
    assert live() == model_only
    del net
    return built


@pytest.mark.parametrize("cycle", [runner_cycle, expert_cycle, dedup_cycle, train_cycle], ids=lambda f: f.__name__)
def test_runner_pieces_give_back_what_they_took(cycle):
    before = live()
    built = []
    for _ in range(2):
        built.append(cycle())
        assert built[-1][0] > before[0] and built[-1][1] > before[1]
        assert live() == before
    assert built[0] == built[1]
