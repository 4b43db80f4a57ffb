"""Plain Python / numpy restatement of the collision shield's spec on top of the PIBT restatement
(tests/expert_ref.py) -- TEST INFRASTRUCTURE ONLY, written from the spec, not from the kernel.

The shield is section 20's PIBT with another candidate order: expert_ref.gen runs unchanged and takes the order through its `rule` hook
(order(a, C) re-sorts section 20's candidates by the policy's preference; pull does nothing).

    ref = RefShield(grids, n_inst, n_agents, max_episode_steps)
    ref.reset(pos, goal)
    actions, planned = ref.step(logit_bits, first)      # uint32 [inst, agent, 5] fp32 bit patterns, int [inst, agent]

State after any number of steps: ref.pos, ref.since, ref.done, ref.overrides.
"""
import numpy as np

from tests import expert_ref as er


def monotone(bits):
    """The monotone map of an fp32 bit pattern to u32: bits ^ 0x80000000 for a clear sign bit, ~bits otherwise."""
    bits = int(bits) & 0xFFFFFFFF
    return (~bits) & 0xFFFFFFFF if bits & 0x80000000 else bits ^ 0x80000000


def bits_of(logits):
    """float32 array -> its bit patterns, uint32 (no floating-point arithmetic touches them afterwards)."""
    return np.ascontiguousarray(logits, dtype=np.float32).view(np.uint32)


def preference(actions, first, bits):
    """The candidate actions `actions` in the order they are tried: `first` first if it is one of them, the others by descending
    monotone(bits[k]), ties by ascending k."""
    head = [k for k in actions if k == int(first)]
    rest = sorted((k for k in actions if k != int(first)), key=lambda k: (-monotone(bits[k]), k))
    return head + rest


def make_rule(first, bits):
    """The `rule` argument of expert_ref.gen for one instance: first [agent], bits [agent][5]."""
    class Rule:
        def __init__(self, *state):
            pass

        def order(self, a, C):
            by_action = {k: c for c in C for k in [c[1]]}
            return [by_action[k] for k in preference(sorted(by_action), first[a], bits[a])], None

        def pull(self, a, j, took_first):
            pass
    return Rule


def plan(grid, pos, dist, since, first, bits):
    """One shield step of one instance -> (next cells [n] of (r, c), actions [n])."""
    nxt, act, _ = er.gen(grid, pos, dist, since, er.priority_order(since), (), 0, 0, 0, make_rule(first, bits))
    return nxt, act


def candidate_actions(grid, pos, dist, a):
    """Section 20's candidate test for agent a: the actions whose cell is in the frame, free and reachable from a's goal."""
    return sorted(k for _, k, _ in er.candidates(grid, pos, dist, {}, 0, 0, 0, a))


def is_collision_free(grid, pos, dist, first):
    """Property 2's premise: every first[a] a candidate, targets pairwise distinct, no edge swap (rotations allowed)."""
    n = len(pos)
    cur = [(int(p[0]), int(p[1])) for p in pos]
    if any(int(first[a]) not in candidate_actions(grid, pos, dist, a) for a in range(n)):
        return False
    tgt = [(cur[a][0] + er.MOVES[int(first[a])][0], cur[a][1] + er.MOVES[int(first[a])][1]) for a in range(n)]
    if len(set(tgt)) != n:
        return False
    where = {c: a for a, c in enumerate(cur)}
    return not any(tgt[a] != cur[a] and tgt[a] in where and tgt[where[tgt[a]]] == cur[a] for a in range(n))


class RefShield(er.RefExpert):
    """RefExpert's state and env; a step takes the policy's logits (as bit patterns) and sampled actions."""

    def __init__(self, grids, n_inst, n_agents, max_episode_steps):
        super().__init__(grids, n_inst, n_agents, max_episode_steps, 0, 0)

    def reset(self, pos, goal):
        super().reset(pos, goal)
        self.overrides = np.zeros(self.n_inst, np.int64)

    def step(self, bits, first, live=None):
        """bits uint32 [inst, agent, >= 5], first [inst, agent]; live: the instances handled (default: all).  For an instance that is done or
        not handled the returned actions are `first`, the returned cells its current ones, and nothing of its state moves."""
        n_inst, n = self.n_inst, self.n_agents
        bits = np.asarray(bits).reshape(n_inst, n, -1)
        first = np.asarray(first).reshape(n_inst, n)
        actions = first.astype(np.int32).copy()
        planned = self.pos.astype(np.int16).copy()
        for i in (range(n_inst) if live is None else live):
            if self.done[i]:
                continue
            grid = self.grid(i)
            nxt, act = plan(grid, self.pos[i], self.dist[i], self.since[i], first[i], bits[i])
            actions[i], planned[i] = act, np.asarray(nxt, np.int16)
            self.overrides[i] += int((np.asarray(act) != first[i]).sum())
            self.pos[i] = np.asarray(er.env_step(grid, self.pos[i], act), np.int64)
            self.tcount[i] += 1
            on = (self.pos[i] == self.goal[i]).all(-1)
            self.since[i] = np.where(on, 0, self.since[i] + 1)
            if on.all():
                self.done[i] = 1
            elif self.tcount[i] >= self.max_steps:
                self.done[i] = 2
        self.t += 1
        return actions, planned


# ---- the hand-written bit patterns both test files use ------------------------------------------------------------------------
NEG_ZERO, POS_ZERO = 0x80000000, 0x00000000
POS_INF, NEG_INF, QNAN, NEG_QNAN = 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000
ONE, TWO, MINUS_ONE = 0x3F800000, 0x40000000, 0xBF800000


def hand_patterns():
    """name -> (bits [5], first, candidate actions, the expected order)."""
    every = [0, 1, 2, 3, 4]
    return {
        "equal_logits": ([ONE] * 5, 2, every, [2, 0, 1, 3, 4]),                                     # ties by ascending k behind first
        "neg_zero_below_pos_zero": ([NEG_ZERO, POS_ZERO, NEG_ZERO, POS_ZERO, MINUS_ONE], 4, every, [4, 1, 3, 0, 2]),
        "infinities": ([POS_INF, NEG_INF, ONE, TWO, MINUS_ONE], 2, every, [2, 0, 3, 4, 1]),
        "nan_has_a_place": ([ONE, QNAN, NEG_QNAN, POS_INF, NEG_INF], 0, every, [0, 1, 3, 4, 2]),    # +NaN above +inf, -NaN below -inf
        "first_into_a_wall": ([ONE, TWO, MINUS_ONE, POS_ZERO, NEG_ZERO], 1, [0, 2, 3, 4], [0, 3, 4, 2]),
        "first_not_the_argmax": ([MINUS_ONE, TWO, ONE, POS_ZERO, NEG_ZERO], 3, every, [3, 1, 2, 4, 0]),
    }


def random_logits(rng, n_inst, n_agents, width=5):
    """Seeded float32 logits whose bit patterns repeat often (ties) and carry the special values now and then."""
    vals = rng.integers(-3, 4, size=(n_inst, n_agents, width)).astype(np.float32) * np.float32(0.5)
    bits = vals.view(np.uint32).copy()
    special = np.array([NEG_ZERO, POS_INF, NEG_INF, QNAN, NEG_QNAN], np.uint32)
    hit = rng.random(size=bits.shape) < 0.05
    bits[hit] = special[rng.integers(0, len(special), size=int(hit.sum()))]
    return bits
