"""The expert's kernels against their restatements at the shapes the other files leave out (tests/expert_shapes.py): 64, 128, 129 and
192 agents on non-square maps (one case with two grids and a shard offset), the dataset recipe's maze with 4 x 32 agents, the
warehouse with 192 and Berlin with 24, a corridor whose distances to the goal exceed a byte, and a map without the wall border.  Each
case runs in four modes -- plain PIBT, PIBT with the swap rule, the search without and with the rule -- under the per-step comparison
and the metric rules of tests/test_gpu_expert.py and test_gpu_expert_swap.py: actions, planned cells, env positions and done flags
after every step, logs, lengths and metrics at the end, and in the search modes status, iterations, nodes, length and solution.

BatchedTokenizer does not refuse a map without the border: its BFS, its row headers and the planner's candidates test the frame, and
nothing here generates observations, so the `frame` case stays.

Every case asserts on the restatement that it is not idle: every instance moves, and at every step some live instance makes a
non-wait action.  (Per instance AND per step does not hold for the maze the recipe fixes: without the swap rule its instance 3 is in
a full deadlock from step 52 on, every agent waiting -- which the device must reproduce as well.)"""
import pytest

from tests import expert_shapes as es
from tests.test_gpu_expert_search import assert_search_equals
from tests.test_gpu_expert_swap import assert_every_step_equals, make_expert

pytestmark = pytest.mark.gpu
CASES = es.shape_cases()


@pytest.mark.parametrize("mode", sorted(es.MODES))
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_step_equals_the_restatement(name, mode):
    case, m = CASES[name], es.MODES[mode]
    ex = make_expert(case, search=m["search"], swap=m["swap"])
    ref = es.run_mode(case, mode, steps=0)
    if name == "serpentine":                                    # the tokenizer's one-byte fields are off: the expert may read the 16-bit ones only
        assert max(int(d[d != 65535].max()) for d in ref.dist[0]) > 255
    if m["search"]:
        assert_search_equals(ex, ref)
    assert_every_step_equals(ex, ref, case["steps"])
    # the case is not vacuous (asserted on the restatement, which the device has just been found equal to)
    es.assert_not_idle(ref)
    if name == "maze32" and m["swap"]:
        assert {"swap", "pull", "clear", "pull_decided"} <= set(ref.trace)
    if name == "frame":
        H, W = case["grids"].shape[1:]
        edge = lambda p: (p[..., 0] == 0) | (p[..., 0] == H - 1) | (p[..., 1] == 0) | (p[..., 1] == W - 1)
        assert edge(case["pos"]).any() and edge(ref.pos).any()  # agents stand on the frame's edge at the start and at the end
