"""Plain Python restatement of the collision shield on lifelong episodes -- TEST INFRASTRUCTURE ONLY, written
from the spec, by composition and with no loop of its own: the lifelong restatement (tests/expert_lifelong_ref.py: the env's restart
rule, the field of a new goal, `since` against the goal held during the step, the arrivals of every step) whose plan of an instance is
the shield's (tests/shield_ref.py: section 20's generator on the policy's preference order).

    ref = RefShieldLifelong(grids, n_inst, n_agents, max_episode_steps)
    ref.reset(pos, goal, queue)                         # queue [inst, agent, Q, 2]
    actions, planned = ref.step(logit_bits, first)      # uint32 [inst, agent, >= 5] fp32 bit patterns, int [inst, agent]

State after any number of steps: RefLifelongExpert's (pos, goal, since, done, reached, arrivals, ...) and ref.overrides.  For an instance
that is done the returned actions are 0 and the returned cells its current ones (the device leaves such an instance's actions as the
caller wrote them).

It also holds the logits both test files feed: goal_seeking_logits() and step_inputs().  A random policy hardly ever arrives, so the
logits seek the goal with noise; they are made step by step from the restatement's own state and handed to both sides.
"""
import numpy as np

from tests import expert_lifelong_ref as lr
from tests import expert_ref as er
from tests import shield_ref as sr

SEED = 8                                              # of step_inputs' generator in both test files (chosen on the CPU: DESIGN.md section 35)


class RefShieldLifelong(lr.RefLifelongExpert):
    def __init__(self, grids, n_inst, n_agents, max_episode_steps):
        super().__init__(grids, n_inst, n_agents, max_episode_steps, 0, 0, swap=False)

    def reset(self, pos, goal, queue):
        super().reset(pos, goal, queue)
        self.overrides = np.zeros(self.n_inst, np.int64)
        self._bits = self._first = None

    def plan_instance(self, i):
        """Section 31's plan on pos, the fields of the goals held now, since, first and the five logits."""
        nxt, act = sr.plan(self.grid(i), self.pos[i], self.dist[i], self.since[i], self._first[i], self._bits[i])
        self.overrides[i] += int((np.asarray(act) != self._first[i]).sum())
        return nxt, act

    def step(self, bits, first):
        self._bits = np.asarray(bits).reshape(self.n_inst, self.n_agents, -1)
        self._first = np.asarray(first).reshape(self.n_inst, self.n_agents)
        return super().step()


def new_ref(case):
    ref = RefShieldLifelong(case["grids"], case["n_inst"], case["n_agents"], case["steps"])
    ref.reset(case["pos"], case["goal"], case["queue"])
    return ref


def cases():
    """The non-swap shapes of expert_lifelong_ref.gpu_cases()."""
    return {name: case for name, case in lr.gpu_cases().items() if not case["swap"]}


def goal_seeking_logits(ref, rng, width=5):
    """-> (bits uint32 [inst, agent, width], first int64 [inst, agent]) from the restatement's state.  For agent a and k = 0..4 the logit
    is -min(dist[a][u_k], 200) where u_k = pos[a] + move[k] passes section 20's candidate test, else -250; a seeded integer of {-1, 0, 1}
    times 0.5 is added to each; `first` is the argmax (lowest k on ties) with probability 0.75, else a seeded action of 0..4.  Columns
    beyond the fifth (never read by the shield) are seeded noise."""
    n_inst, n = ref.n_inst, ref.n_agents
    logits = np.full((n_inst, n, width), -250.0, np.float32)
    for i in range(n_inst):
        grid = ref.grid(i)
        for a in range(n):
            for k in sr.candidate_actions(grid, ref.pos[i], ref.dist[i], a):
                u = (int(ref.pos[i, a, 0]) + er.MOVES[k][0], int(ref.pos[i, a, 1]) + er.MOVES[k][1])
                logits[i, a, k] = -float(min(int(ref.dist[i][a][u]), 200))
    logits[..., 5:] = 0.0
    logits += rng.integers(-1, 2, size=logits.shape).astype(np.float32) * np.float32(0.5)
    best = logits[..., :5].argmax(-1)
    other = rng.integers(0, 5, size=(n_inst, n))
    first = np.where(rng.random(size=(n_inst, n)) < 0.75, best, other)
    return sr.bits_of(logits).copy(), first.astype(np.int64)


def step_inputs(ref, rng, t, width=None):
    """The inputs of step t: goal-seeking logits, and on every 7th step (t % 7 == 6) shield_ref.random_logits with a seeded `first` of
    0..4, so that the special bit patterns (ties, -0, infinities, NaNs) occur in a lifelong episode too.  width None: rows of 7 logits on
    even steps and of 5 on odd ones (ld > 5: only the first five values of a row are read)."""
    width = (5 if t % 2 else 7) if width is None else width
    if t % 7 == 6:
        return sr.random_logits(rng, ref.n_inst, ref.n_agents, width), rng.integers(0, 5, size=(ref.n_inst, ref.n_agents)).astype(np.int64)
    return goal_seeking_logits(ref, rng, width)
