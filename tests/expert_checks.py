"""An independent checker of expert output -- TEST INFRASTRUCTURE ONLY.  Plain numpy over all instances at once, written from the MAPF
invariants of DESIGN.md section 20 and the episode rules of section 4; it imports nothing from the restatements (tests/expert_ref.py,
expert_search_ref.py, expert_swap_ref.py), so a mistake a restatement shares with its kernel does not pass here.

    check_transition(grids, pos, actions, planned, pos_after, skip)      # AssertionError naming the first offender
    final_pos, metrics = replay(grids, pos0, goal, log, lens)            # through the C oracle's env step
    trajectory_metrics(traj, goal)                                       # CSR, ISR, SoC, makespan, ep_length of one episode
"""
import numpy as np

MOVES = np.array([(0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)], np.int64)       # 0 wait, 1 up, 2 down, 3 left, 4 right


def _fail(bad, what):
    """bad: bool [inst] or [inst, agent]; raise on the first True entry."""
    if bad.any():
        where = np.argwhere(bad)[0].tolist()
        names = ("instance", "agent")
        raise AssertionError(what + " (" + ", ".join(f"{k} {v}" for k, v in zip(names, where)) + f"; {int(bad.sum())} in all)")


def check_transition(grids, pos, actions, planned, pos_after, skip):
    """One step of every instance.  grids [n_grids, H, W] (non-zero = blocked; instance i stands on grid i % n_grids), pos, planned and
    pos_after [inst, agent, 2], actions [inst, agent], skip bool [inst].  For every instance that is not skipped: the planned cells are
    pairwise distinct; every planned cell is a free cell of the instance's grid; planned = pos + MOVES[action] with action in 0..4; no
    two agents exchange cells; pos_after = planned (the env executed the plan).  For a skipped (done) instance: every action is 0 and
    planned = pos."""
    grids = np.asarray(grids)
    if grids.ndim == 2:
        grids = grids[None]
    n_grids, H, W = grids.shape
    pos, planned, pos_after = (np.asarray(x).astype(np.int64) for x in (pos, planned, pos_after))
    actions = np.asarray(actions).astype(np.int64)
    n_inst, n = actions.shape
    assert pos.shape == planned.shape == pos_after.shape == (n_inst, n, 2)
    skip = np.asarray(skip).astype(bool).reshape(n_inst)
    live = ~skip[:, None]

    _fail(skip[:, None] & (actions != 0), "a skipped instance has a non-zero action")
    _fail(skip[:, None] & (planned != pos).any(-1), "a skipped instance plans to leave its cell")

    in_frame = (planned[..., 0] >= 0) & (planned[..., 0] < H) & (planned[..., 1] >= 0) & (planned[..., 1] < W)
    _fail(live & ~in_frame, "blocked cell: a planned cell lies outside the frame")
    r, c = np.where(in_frame, planned[..., 0], 0), np.where(in_frame, planned[..., 1], 0)
    g = (np.arange(n_inst) % n_grids)[:, None]
    _fail(live & (grids[g, r, c] != 0), "blocked cell: a planned cell is not free")

    pc, cc = planned[..., 0] * W + planned[..., 1], pos[..., 0] * W + pos[..., 1]
    if n > 1:
        order = np.argsort(pc, axis=1, kind="stable")
        srt = np.take_along_axis(pc, order, 1)
        dup = np.zeros((n_inst, n), bool)
        np.put_along_axis(dup, order[:, 1:], srt[:, 1:] == srt[:, :-1], 1)
        _fail(live & dup, "vertex conflict: two agents plan the same cell")

    owner = np.full((n_inst, H * W), -1, np.int64)                           # who stands on a cell now
    rows = np.arange(n_inst)[:, None]
    owner[rows, cc] = np.arange(n)[None, :]
    b = owner[rows, pc]                                                      # the agent standing on my planned cell
    other = (b >= 0) & (b != np.arange(n)[None, :])
    back = np.take_along_axis(pc, np.where(other, b, 0), 1) == cc            # ... plans my cell
    _fail(live & other & back, "edge swap: two agents exchange cells")

    bad_act = (actions < 0) | (actions > 4)
    _fail(live & bad_act, "action outside 0..4")
    _fail(live & (planned != pos + MOVES[np.where(bad_act, 0, actions)]).any(-1), "the action does not match the move: planned != pos + MOVES[action]")

    _fail(live & (pos_after != planned).any(-1), "the env left an agent off its planned cell: pos_after != planned")


def trajectory_metrics(traj, goal):
    """One episode's CSR, ISR, SoC, makespan, ep_length (float64 [5]) from its whole trajectory, by the rules of DESIGN.md section 4 and
    not by the env kernel's incremental bookkeeping.  traj [steps + 1, agent, 2]: the cells at reset and after every step made; goal
    [agent, 2].  The episode ends at the first step after which every agent stands on its goal, else with the last step given; an
    agent's arrival time is the start of its final uninterrupted stay on the goal (0 if it never left it), ep_length if it does not end
    there."""
    traj, goal = np.asarray(traj).astype(np.int64), np.asarray(goal).astype(np.int64)
    on = (traj == goal[None]).all(-1)                                        # [steps + 1, agent]
    ends = np.flatnonzero(on[1:].all(1))
    T = int(ends[0]) + 1 if len(ends) else len(traj) - 1
    on = on[:T + 1]
    off = np.where(~on, np.arange(T + 1)[:, None], -1).max(0)                # the last time the agent was off its goal, -1 = never
    arrive = np.where(on[T], off + 1, T)
    return np.array([float(on[T].all()), float(on[T].mean()), float(arrive.sum()), float(arrive.max()), float(T)])


def replay(grids, pos0, goal, log, lens):
    """Step every instance through the C oracle's env (oracle.env_step) with its own lens[i] logged actions.
    grids [n_grids, H, W], pos0 and goal [inst, agent, 2], log [inst, agent, T], lens [inst].
    -> (final positions int64 [inst, agent, 2], float64 [inst, 5] = CSR, ISR, SoC, makespan, ep_length of the trajectories)."""
    from oracle import oracle as orc
    grids = np.asarray(grids)
    if grids.ndim == 2:
        grids = grids[None]
    pos0, goal, log, lens = np.asarray(pos0), np.asarray(goal), np.asarray(log), np.asarray(lens)
    n_inst = pos0.shape[0]
    final = np.empty(pos0.shape, np.int64)
    metrics = np.empty((n_inst, 5))
    for i in range(n_inst):
        grid, g = grids[i % len(grids)], goal[i].astype(np.int32)
        p = pos0[i].astype(np.int32)
        traj = [p]
        for t in range(int(lens[i])):
            p, _ = orc.env_step(grid, p, g, log[i, :, t].astype(np.int32))
            traj.append(p)
        final[i] = p
        metrics[i] = trajectory_metrics(np.stack(traj), g)
    return final, metrics
