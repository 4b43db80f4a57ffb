"""Dataset-side bulk tokenizer on the device: host mirror of the reference's
`dataset/tokenizer/generate_observations.py:ObservationGenerator` (same constructor arguments, same
`generate_observations(start_range, end_range) -> (inputs, gt_actions)`), over `mgpt_dataset_*`.

    gen = ObservationGenerator(maps, data, cfg)          # maps: {name: map string}, data: list of logged instances
    inputs, gt_actions = gen.generate_observations(0, len(data))

`data[i]` = {"metrics": {"CSR", "made_actions", "init_positions"}, "env_grid_search": {"map_name"}} (the
toolbox's result records, generate_observations.py:43-66).  Instances with CSR < 1 are skipped (:44-45); the
all-pairs distance table of a map is built once and reused while consecutive instances share the map (:46-54).
Lifelong logs ("global_lifelong_targets_xy", :55-60, 143-153) and the `mask_cost2go` ablation (:253-262) are handled on the
device like the rest; the other three mask_* fields are carried by `InputParameters` but, as in the reference's dataset
pipeline (whose C++ encoder ignores them), only the python `Encoder.mask` applies them (tokenizer.py:104-138; restated for the tests in oracle/dataset_encoder.py).
Not supported: cost2go_radius != 5.

Batched route: `tokenize_episodes(table, init, actions, lengths, ...)` turns a whole batch of episodes of one map --
the expert's device log as BatchedExpert.log() returns it -- into (rows, labels, row0) on the device in one call, with no per-episode
host work; `TableCache` keeps the maps' all-pairs tables by grid bytes.  BatchedExpert.dataset_rows and dataset_build.EpisodeStore sit on
top of the two.  `episode_row_offsets` / `episode_labels` restate the offsets and the label rule in numpy (tests, tools).
Lifelong logs take the same route: `tokenize_episodes(..., targets=, n_targets=)` hands the agents' target lists
(goal at reset + cyclic queue, as BatchedExpert.lifelong_targets() returns them) to mgpt_dataset_tokenize_episodes_lifelong, which
derives the goal of every timestep on the device; `episode_goals` restates that rule in numpy.  BatchedExpert.lifelong_rows and
dataset_build.EpisodeStore(lifelong=True) sit on top of it.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib, maps as _maps

MOVES = np.array([[0, 0], [-1, 0], [1, 0], [0, -1], [0, 1]], dtype=np.int32)      # generate_observations.py:10


class InputParameters:
    """= dataset/tokenizer/parameters.py (field names and defaults)."""

    def __init__(self, num_agents=13, num_previous_actions=5, agents_radius=5, cost2go_value_limit=20, cost2go_radius=5,
                 context_size=256, mask_greed_action=False, mask_actions_history=False, mask_goal=False, mask_cost2go=False):
        if (num_agents, num_previous_actions, agents_radius, cost2go_value_limit, cost2go_radius, context_size) != (13, 5, 5, 20, 5, 256):
            raise NotImplementedError("only the reference's defaults (13, 5, 5, 20, 5, 256) are implemented")
        self.mask_greed_action, self.mask_actions_history = bool(mask_greed_action), bool(mask_actions_history)
        self.mask_goal, self.mask_cost2go = bool(mask_goal), bool(mask_cost2go)
        self.num_agents, self.num_previous_actions, self.agents_radius = num_agents, num_previous_actions, agents_radius
        self.cost2go_value_limit, self.cost2go_radius, self.context_size = cost2go_value_limit, cost2go_radius, context_size


class MapTable:
    """All-pairs BFS table of one padded map on the device (the reference's cost2go_data, cost2go.cpp:33-42)."""

    def __init__(self, grid_padded, device="cuda"):
        _lib.require_gpu()
        self.device = torch.device(device)
        g = torch.as_tensor(np.ascontiguousarray(np.asarray(grid_padded) != 0, dtype=np.uint8)).to(self.device)
        self.H, self.W = g.shape
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mgpt_dataset_create(ctypes.byref(self._h), _lib.ptr(g), self.H, self.W, _lib.stream_ptr()))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                _lib.lib().mgpt_dataset_destroy(h)
            except Exception:
                pass
            self._h = None

    def tokenize(self, paths, goals=None, mask_cost2go=False):
        """paths int16 [n_agents, n_steps, 2] (padded coords) -> uint8 device tensor [n_agents, n_steps, 256].
        goals (lifelong logs): int16 [n_agents, n_steps, 2], the goal pursued at every timestep; mask_cost2go: the
        window shows blocked / free only (cost2go.cpp:52-62)."""
        p = torch.as_tensor(np.ascontiguousarray(paths, dtype=np.int16)).to(self.device)
        n, T1 = int(p.shape[0]), int(p.shape[1])
        g = None
        if goals is not None:
            g = torch.as_tensor(np.ascontiguousarray(goals, dtype=np.int16)).to(self.device)
            assert tuple(g.shape) == (n, T1, 2), "goals must have the shape of paths"
        out = torch.empty((n, T1, 256), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mgpt_dataset_tokenize_ex(self._h, n, T1, _lib.ptr(p), _lib.ptr(g) if g is not None else None,
                                                           1 if mask_cost2go else 0, _lib.ptr(out), _lib.stream_ptr()))
        return out


def agent_paths(init_positions, made_actions):
    """= get_agent_paths (:159-177): [n][T+1][2] cells after every logged action."""
    acts = np.asarray(made_actions, dtype=np.int64)
    steps = MOVES[acts]                                                 # [n, T, 2]
    p0 = np.asarray(init_positions, dtype=np.int32)[:, None, :]
    return np.concatenate([p0, p0 + np.cumsum(steps, axis=1)], axis=1)


def goal_positions(paths, targets):
    """= get_goal_positions (:143-153): the goal at every path cell = the first target of the agent's list it has not stood
    on yet (standing on it advances the list before the cell's goal is read).  -> int32 [n, T+1, 2].
    Like the reference, a path that exhausts its list raises IndexError."""
    out = np.empty_like(np.asarray(paths, dtype=np.int32))
    for a, (path, tg) in enumerate(zip(paths, targets)):
        cur = 0
        for t, pos in enumerate(path):
            if int(pos[0]) == int(tg[cur][0]) and int(pos[1]) == int(tg[cur][1]):
                cur += 1
            out[a, t] = (int(tg[cur][0]), int(tg[cur][1]))
    return out


def gt_actions(made_actions):
    """Labels of generate_observations.py:67-90: the logged action, one appended wait, 5 = "wait in goal" after the last move."""
    out = []
    for acts in made_actions:
        a = list(acts) + [0]
        nz = [i for i, v in enumerate(a) if v != 0]
        goal_t = nz[-1] if nz else len(a)
        out.append([5 if t > goal_t else a[t] for t in range(len(a))])
    return out


def episode_row_offsets(lengths, n_agents, max_steps, keep=None, episodes=None):
    """numpy restatement of mgpt_dataset_episode_offsets: int64 [n_sel + 1], the exclusive scan of
    rows(e) = keep[e] ? n_agents * (clamp(len[e], 0, max_steps) + 1) : 0 over `episodes` (None: all, in order)."""
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    sel = np.arange(len(lengths)) if episodes is None else np.asarray(episodes, dtype=np.int64).reshape(-1)
    rows = int(n_agents) * (np.clip(lengths[sel], 0, int(max_steps)) + 1)
    if keep is not None:
        rows = np.where(np.asarray(keep).reshape(-1)[sel] != 0, rows, 0)
    return np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)


def episode_labels(actions, length):
    """numpy restatement of the device's label rule = gt_actions on one episode's log: actions int8 [n_agents, >= length] (bytes outside
    0..4 count as 0) -> int8 [n_agents, length + 1]: with a = actions[:length] + [0] and g the index of a's last non-zero entry
    (length + 1 if none), 5 where t > g, else a[t]."""
    a = np.asarray(actions).astype(np.int64)[:, :int(length)]
    a = np.where((a >= 0) & (a <= 4), a, 0)
    a = np.concatenate([a, np.zeros((a.shape[0], 1), np.int64)], axis=1)
    t = np.arange(a.shape[1])
    g = np.where((a != 0).any(1), ((a != 0) * t).max(1), a.shape[1])
    return np.where(t[None, :] > g[:, None], 5, a).astype(np.int8)


def target_at(targets, j):
    """target(j) of one agent's list as the lifelong batched call addresses it: targets [L, 2]; entry 0, then the L - 1 entries behind it
    cyclically -- the expert's (goal at reset, cyclic queue) as it lies."""
    L = len(targets)
    return targets[0] if j == 0 else targets[1 + (j - 1) % (L - 1)]


def episode_goals(init, actions, length, targets, n_targets=None):
    """numpy restatement of the device's per-step goal rule (= goal_positions, with the cyclic addressing of
    mgpt_dataset_tokenize_episodes_lifelong) on one episode's log: init [n_agents, 2], actions int8 [n_agents, >= length] (bytes outside 0..4
    count as 0), targets int16 [n_agents, L, 2], n_targets [n_agents] or None (L each) -> int32 [n_agents, length + 1, 2].  Walking an agent's
    path t = 0 .. length with cur = 0: a cell equal to target(cur) advances cur (an `if`; also at t = 0), the goal at t is target(cur).
    A walk that reaches n_targets raises IndexError, as the reference does."""
    a = np.asarray(actions).astype(np.int64)[:, :int(length)]
    a = np.where((a >= 0) & (a <= 4), a, 0)
    paths = agent_paths(np.asarray(init).reshape(-1, 2), a)
    targets = np.asarray(targets).astype(np.int32)
    n, L = int(targets.shape[0]), int(targets.shape[1])
    assert targets.shape == (paths.shape[0], L, 2) and L >= 1, "targets [n_agents, L >= 1, 2]"
    nt = np.full((n,), L, np.int64) if n_targets is None else np.asarray(n_targets, dtype=np.int64).reshape(n)
    out = np.empty_like(paths)
    for ag in range(n):
        limit = min(int(nt[ag]), 1) if L == 1 else int(nt[ag])
        cur = 0
        if limit < 1:
            raise IndexError(f"agent {ag}: an empty target list")
        for t in range(paths.shape[1]):
            if (paths[ag, t] == target_at(targets[ag], cur)).all():
                cur += 1
                if cur >= limit:
                    raise IndexError(f"agent {ag} exhausts its {limit} targets at t = {t}")
            out[ag, t] = target_at(targets[ag], cur)
    return out


def tokenize_episodes(table, init, actions, lengths, keep=None, episodes=None, mask_cost2go=False, max_rows_per_call=1 << 22,
                      targets=None, n_targets=None):
    """A batch of logged episodes of one map -> (rows uint8 [N, 256], labels int8 [N], row0 int64 [n_sel + 1]), device tensors.
    table: the map's MapTable (the episodes' frame); init int16 [n_batch, n_agents, 2] first cells in its coordinates; actions int8
    [n_batch, n_agents, max_steps] and lengths int32 [n_batch] as BatchedExpert.log() returns them; keep: uint8 / bool [n_batch] or
    None, 0 = the episode gives no rows; episodes: the selected episodes in output order (list, array or tensor of indices below
    n_batch) or None for all.  Selected episode k owns rows [row0[k], row0[k + 1]): what MapTable.tokenize makes of its paths, agent-major
    then timestep 0 .. len, with the labels of gt_actions.  The one value read back is row0[-1], to size the output (with `episodes` on
    the device, a flag that every index is in range travels with it).  The selection is tokenized in pieces of at most max_rows_per_call //
    (n_agents * (max_steps + 1)) episodes (at least one), which bounds the library's workspace; the result does not depend on the pieces.
    targets (lifelong logs): int16 [n_batch, n_agents, L, 2], every agent's target list -- entry 0, then the L - 1
    entries behind it cyclically (BatchedExpert.lifelong_targets(); a plain list is the case without a wrap); n_targets int32 [n_batch,
    n_agents] or None (L each), the lists' lengths.  The records then carry the goal pursued at every timestep (episode_goals) and the rows
    are what MapTable.tokenize(paths, goals) makes of the episode.  One more value is read back then, after the last piece: a flag that a
    kept agent's walk exhausted its list, which raises IndexError as the reference does."""
    dev = table.device
    init = torch.as_tensor(init).to(dev, torch.int16).contiguous()
    actions = torch.as_tensor(actions).to(dev, torch.int8).contiguous()
    lengths = torch.as_tensor(lengths).to(dev, torch.int32).contiguous()
    assert actions.dim() == 3 and tuple(init.shape) == tuple(actions.shape[:2]) + (2,) and tuple(lengths.shape) == (actions.shape[0],), \
        "init [n_batch, n_agents, 2], actions [n_batch, n_agents, max_steps], lengths [n_batch]"
    n_batch, n_agents, max_steps = (int(v) for v in actions.shape)
    if keep is not None:
        keep = (torch.as_tensor(keep).to(dev) != 0).to(torch.uint8).contiguous()
        assert tuple(keep.shape) == (n_batch,), "keep [n_batch]"
    if targets is None:
        assert n_targets is None, "n_targets needs targets"
    else:
        targets = torch.as_tensor(targets).to(dev, torch.int16).contiguous()
        assert targets.dim() == 4 and tuple(targets.shape[:2]) == (n_batch, n_agents) and targets.shape[2] >= 1 and targets.shape[3] == 2, \
            "targets [n_batch, n_agents, L >= 1, 2]"
        if n_targets is not None:
            n_targets = torch.as_tensor(n_targets).to(dev, torch.int32).contiguous()
            assert tuple(n_targets.shape) == (n_batch, n_agents), "n_targets [n_batch, n_agents]"
    flag = None
    if episodes is None:
        n_sel = n_batch
    elif torch.is_tensor(episodes) and episodes.is_cuda:
        raw = episodes.to(dev, torch.int64).reshape(-1)
        n_sel = int(raw.shape[0])
        episodes = raw.clamp(0, max(n_batch - 1, 0)).to(torch.int32).contiguous()
        flag = (episodes != raw).any().to(torch.int64).reshape(1)
    else:
        host = np.asarray(episodes.cpu() if torch.is_tensor(episodes) else episodes, dtype=np.int64).reshape(-1)
        if len(host) and (host.min() < 0 or host.max() >= n_batch):
            raise IndexError(f"episodes outside 0 .. {n_batch - 1}")
        n_sel = len(host)
        episodes = torch.as_tensor(host.astype(np.int32)).to(dev)
    row0 = torch.empty((n_sel + 1,), dtype=torch.int64, device=dev)
    L = _lib.lib()
    with _lib.on_device(dev):
        s = _lib.stream_ptr()
        _lib.check(L.mgpt_dataset_episode_offsets(n_sel, n_agents, max_steps, _lib.ptr(lengths), _lib.ptr(keep) if keep is not None else None,
                                                  _lib.ptr(episodes) if episodes is not None else None, _lib.ptr(row0), s))
        back = (row0[-1:] if flag is None else torch.cat([row0[-1:], flag])).cpu().tolist()
        if flag is not None and back[1]:
            raise IndexError(f"episodes outside 0 .. {n_batch - 1}")
        n_rows = int(back[0])
        rows = torch.empty((n_rows, 256), dtype=torch.uint8, device=dev)
        labels = torch.empty((n_rows,), dtype=torch.int8, device=dev)
        if n_rows == 0:
            return rows, labels, row0
        per = max(1, int(max_rows_per_call) // (n_agents * (max_steps + 1)))
        if per < n_sel and episodes is None:                 # a piece names its episodes: k of a window is not the episode's index
            episodes = torch.arange(n_sel, dtype=torch.int32, device=dev)
        status = torch.zeros((1,), dtype=torch.int32, device=dev) if targets is not None else None
        for k0 in range(0, n_sel, per):
            k1 = min(k0 + per, n_sel)
            piece = (table._h, k1 - k0, n_agents, max_steps, _lib.ptr(init), _lib.ptr(actions), _lib.ptr(lengths),
                     _lib.ptr(keep) if keep is not None else None,
                     ctypes.c_void_p(episodes.data_ptr() + 4 * k0) if episodes is not None else None, ctypes.c_void_p(row0.data_ptr() + 8 * k0))
            out = (1 if mask_cost2go else 0, _lib.ptr(rows), _lib.ptr(labels), s)
            if targets is None:
                _lib.check(L.mgpt_dataset_tokenize_episodes(*piece, *out))
            else:
                _lib.check(L.mgpt_dataset_tokenize_episodes_lifelong(*piece, _lib.ptr(targets), int(targets.shape[2]),
                                                                     _lib.ptr(n_targets) if n_targets is not None else None,
                                                                     _lib.ptr(status), *out))
        if status is not None and status.cpu().item():
            raise IndexError("a kept episode's agent stood on more targets than its list holds (generate_observations.py:146-149)")
    return rows, labels, row0


class TableCache:
    """grid bytes -> MapTable, within a byte budget (a table is 2 * (H * W) ** 2 bytes), oldest first out.  The key is the frame grid
    itself, as the expert holds it -- not a map name or string: a frame larger than the map's own padded grid only adds blocked cells,
    which the table and the window both treat as unreachable, so the rows are those of the map's own grid.
    The newest table stays even when it alone exceeds the budget.  make(grid, device) builds a table (tests count the builds)."""

    def __init__(self, budget_bytes=8 << 30, device="cuda", make=None):
        self.budget, self.device = int(budget_bytes), device
        self._make = make if make is not None else MapTable
        self._tables = collections.OrderedDict()             # key -> (table, bytes), in order of creation
        self.bytes = self.builds = 0

    @staticmethod
    def key(grid):
        g = np.ascontiguousarray(np.asarray(grid.cpu() if torch.is_tensor(grid) else grid) != 0, dtype=np.uint8)
        assert g.ndim == 2, "grid [H, W]"
        return g.shape + (g.tobytes(),), g

    def __len__(self):
        return len(self._tables)

    def get(self, grid):
        key, g = self.key(grid)
        hit = self._tables.get(key)
        if hit is not None:
            return hit[0]
        size = 2 * (g.shape[0] * g.shape[1]) ** 2
        while self._tables and self.bytes + size > self.budget:
            _, (_, freed) = self._tables.popitem(last=False)
            self.bytes -= freed
        table = self._make(g, self.device)
        self._tables[key] = (table, size)
        self.bytes += size
        self.builds += 1
        return table


class ObservationGenerator:
    def __init__(self, maps, data, cfg=None, device="cuda"):
        self.cfg = cfg or InputParameters()
        self.maps, self.data, self.device = maps, data, device
        self.inputs, self.gt_actions = [], []
        self._table, self._table_name = None, None

    def get_grid_map(self, map_name):
        """= :105-119: '.'/'#' string -> padded 0/1 array."""
        rows = [r for r in self.maps[map_name].split() if r]
        for i, r in enumerate(rows):
            bad = set(r) - {".", "#"}
            if bad:
                raise KeyError(f"Unsupported symbol '{sorted(bad)[0]}' at line {i}")            # :101
        obst = np.array([[1 if ch == "#" else 0 for ch in r] for r in rows], dtype=np.uint8)
        return _maps.pad(obst, self.cfg.cost2go_radius, 1)

    def _instances(self, start_range, end_range):
        """Per kept instance of data[start_range:end_range], in order: (uint8 device tensor [rows, 256], its labels as a list)."""
        for instance_id in range(start_range, end_range):
            rec = self.data[instance_id]
            if rec["metrics"].get("CSR", 1) < 1:                        # :44-45
                continue
            name = rec["env_grid_search"]["map_name"]
            if name != self._table_name:                                # :46-54
                self._table, self._table_name = MapTable(self.get_grid_map(name), self.device), name
            paths = agent_paths(rec["metrics"]["init_positions"], rec["metrics"]["made_actions"])
            goals = None
            if "global_lifelong_targets_xy" in rec["metrics"]:          # :55-60
                goals = goal_positions(paths, rec["metrics"]["global_lifelong_targets_xy"])
            rows = self._table.tokenize(paths, goals, self.cfg.mask_cost2go).reshape(-1, 256)
            yield rows, [v for g in gt_actions(rec["metrics"]["made_actions"]) for v in g]

    def generate_observations_device(self, start_range, end_range):
        """The rows of `generate_observations` (same instances, order, CSR filter and labels) left where the kernel wrote them:
        -> (uint8 device tensor [N, 256], int8 device tensor [N]).  Only the labels (one byte per row, built from the logged
        actions on the host) travel to the device; no row travels back.  Does not touch self.inputs / self.gt_actions."""
        rows, labels = [], []
        for x, y in self._instances(start_range, end_range):
            rows.append(x)
            labels.extend(y)
        dev = torch.device(self.device)
        if not rows:
            return torch.empty((0, 256), dtype=torch.uint8, device=dev), torch.empty((0,), dtype=torch.int8, device=dev)
        x = rows[0] if len(rows) == 1 else torch.cat(rows)
        y = torch.as_tensor(np.asarray(labels, dtype=np.int8)).to(dev)
        assert x.shape[0] == y.shape[0]
        return x, y

    def generate_observations(self, start_range, end_range):
        self.inputs, self.gt_actions = [], []
        for x, y in self._instances(start_range, end_range):
            self.inputs.extend(list(x.cpu().numpy().astype(np.int8)))
            self.gt_actions.extend(y)
        return self.inputs, self.gt_actions

