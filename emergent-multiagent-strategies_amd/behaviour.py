"""Strategy fingerprints: per match-up cell, integer histograms of what the teams DO -- where the agents of each team stand,
fire and die, how many are alive t steps into an episode, how long episodes last -- summed on the device over the rollout
storage of every chunk (csrc/fa_behaviour.hip; include/fortattack.h: fa_behaviour_begin / fa_behaviour_chunk).

``behaviour_chunk_numpy`` is the definition, statement for statement: the kernel's test reference and its documentation, as
``render.render_frame`` is for fa_render.  ``BehaviourMaps`` drives the device pass; ``fingerprint_rows`` turns the integer
maps into a few floats per match-up on the host; ``write_heatmaps`` draws one cell's maps.

Known limit: with auto-reset the terminal state of an episode never reaches the storage (obs[s + 1] is already the next
episode's reset observation), so a death on the step that ends an episode is not in ``deaths``; ``alive_at_end`` of the match
table (crossplay.crossplay_rows) covers it.
"""
import numpy as np

BX, BY = 40, 32             # include/fortattack.h FA_BEHAVIOUR_BX / _BY
SECTIONS = ("steps", "episodes", "len_hist", "alive_t", "occ", "shots", "deaths")
FINGERPRINT_COLUMNS = ("mean_episode_length", "guard_shots_per_alive_step", "attacker_shots_per_alive_step",
                       "guard_mean_y", "attacker_mean_y", "guard_std_x", "attacker_std_x", "guard_share_near_door",
                       "attacker_share_upper_half", "guard_deaths_per_alive_step", "attacker_deaths_per_alive_step")
# the reference literals (core.py:128, fortattack_env_v1.py:16-17), used where no fa_world_consts is given
_WORLD_KEYS = ("wall_xmin", "wall_xmax", "wall_ymin", "wall_ymax", "fort_dim", "door_x", "door_y")
_REFERENCE_WORLD = dict(wall_xmin=-1.0, wall_xmax=1.0, wall_ymin=-0.8, wall_ymax=0.8, fort_dim=0.15, door_x=0.0, door_y=0.8)


def _world(world):
    """None (the reference literals), a dict or an fa_world_consts (attributes) -> a dict of floats."""
    if world is None:
        return dict(_REFERENCE_WORLD)
    get = world.get if isinstance(world, dict) else lambda k, d: getattr(world, k, d)
    return {k: float(get(k, _REFERENCE_WORLD[k])) for k in _WORLD_KEYS}


def cell_words(max_time_steps):
    """uint64 words of one cell's record (FA_BEHAVIOUR_CELL_WORDS)."""
    return 2 + 3 * int(max_time_steps) + 6 * BY * BX


def section_offsets(max_time_steps):
    """name -> (offset in words, shape) of every section of a cell's record, in record order (FA_BEHAVIOUR_OFF_*)."""
    MT = int(max_time_steps)
    shapes = dict(steps=(), episodes=(), len_hist=(MT,), alive_t=(2, MT), occ=(2, BY, BX), shots=(2, BY, BX), deaths=(2, BY, BX))
    out, at = {}, 0
    for k in SECTIONS:
        out[k] = (at, shapes[k])
        at += int(np.prod(shapes[k], dtype=np.int64))
    assert at == cell_words(MT)
    return out


def new_counts(n_cells, max_time_steps):
    """A zero record: a dict of int64 arrays, each with a leading n_cells axis."""
    return {k: np.zeros((int(n_cells),) + shape, np.int64) for k, (_, shape) in section_offsets(max_time_steps).items()}


def unpack_counts(raw, n_cells, max_time_steps):
    """(n_cells * cell_words) words as the device holds them -> the dict of int64 arrays."""
    raw = np.asarray(raw).reshape(int(n_cells), cell_words(max_time_steps)).astype(np.int64)
    return {k: raw[:, at:at + int(np.prod(shape, dtype=np.int64))].reshape((int(n_cells),) + shape).copy()
            for k, (at, shape) in section_offsets(max_time_steps).items()}


def merge_counts(a, b):
    """Records of shards, ranks or successive evaluations merge by plain addition."""
    return {k: np.asarray(a[k], np.int64) + np.asarray(b[k], np.int64) for k in SECTIONS}


def bin_consts(world=None):
    """(x0, sx, y0, sy) float32: the origin and the bins per world unit of both axes; the quotient is taken in double."""
    w = _world(world)
    return (np.float32(w["wall_xmin"]), np.float32(BX / (w["wall_xmax"] - w["wall_xmin"])),
            np.float32(w["wall_ymin"]), np.float32(BY / (w["wall_ymax"] - w["wall_ymin"])))


def bin_index(v, v0, scale, n):
    """clamp(floor((v - v0) * scale), 0, n - 1): the subtraction and the product are two separately rounded float32
    operations, the clamp is taken in float32 before the conversion to an integer."""
    v = np.asarray(v, np.float32)
    f = np.floor((v - np.float32(v0)) * np.float32(scale))
    return np.clip(f, np.float32(0), np.float32(n - 1)).astype(np.int64)


def behaviour_chunk_numpy(obs, actions, done, cell, ep_count, ep_t, counts, num_guards, max_time_steps, quota=0, world=None):
    """One chunk of the definition.  obs (T+1, E, N, 6) float32 rows [alive, x, y, ang, vx, vy]; actions (T, E, N[, 1]);
    done (T, E); cell (E) the match-up cell of every env; ep_count / ep_t (E) integer arrays, the persistent counters,
    updated IN PLACE like `counts` (new_counts).  For s = 0 .. T-1, in order, for every env e:

        if quota > 0 and ep_count[e] >= quota: stop               # this env has played its episodes
        t = min(ep_t[e], max_time_steps - 1);  team = 0 for guards, 1 for attackers
        for every agent i with obs[s, e, i, 0] != 0:               # alive when it acted
            occ[c][team][by][bx] += 1;  alive_t[c][team][t] += 1
            if actions[s, e, i] == 7:                    shots[c][team][by][bx] += 1
            if not done[s, e] and obs[s+1, e, i, 0] == 0: deaths[c][team][by][bx] += 1
        steps[c] += 1
        if done[s, e]: len_hist[c][t] += 1; episodes[c] += 1; ep_count[e] += 1; ep_t[e] = 0
        else:          ep_t[e] += 1

    An env whose cell is outside [0, n_cells) is scanned (its counters advance) and counted nowhere."""
    obs = np.asarray(obs, np.float32)
    T, E, N = obs.shape[0] - 1, obs.shape[1], obs.shape[2]
    actions = np.asarray(actions).reshape(T, E, N)
    done = np.asarray(done).reshape(T, E) != 0
    cell = np.asarray(cell, np.int64).reshape(E)
    n_cells, MT, G, quota = counts["steps"].shape[0], int(max_time_steps), int(num_guards), int(quota)
    x0, sx, y0, sy = bin_consts(world)
    team = (np.arange(N) >= G).astype(np.int64)
    in_cell = (cell >= 0) & (cell < n_cells)
    for s in range(T):
        live = np.ones(E, bool) if quota <= 0 else ep_count < quota
        t = np.minimum(ep_t, MT - 1).astype(np.int64)
        tab = live & in_cell                                       # the envs whose step is counted somewhere
        alive = (obs[s, :, :, 0] != 0) & tab[:, None]
        e_idx, i_idx = np.nonzero(alive)
        c = cell[e_idx]
        bx = bin_index(obs[s, e_idx, i_idx, 1], x0, sx, BX)
        by = bin_index(obs[s, e_idx, i_idx, 2], y0, sy, BY)
        np.add.at(counts["occ"], (c, team[i_idx], by, bx), 1)
        np.add.at(counts["alive_t"], (c, team[i_idx], t[e_idx]), 1)
        shot = actions[s, e_idx, i_idx] == 7
        np.add.at(counts["shots"], (c[shot], team[i_idx][shot], by[shot], bx[shot]), 1)
        died = ~done[s, e_idx] & (obs[s + 1, e_idx, i_idx, 0] == 0)
        np.add.at(counts["deaths"], (c[died], team[i_idx][died], by[died], bx[died]), 1)
        np.add.at(counts["steps"], cell[tab], 1)
        ended = tab & done[s]
        np.add.at(counts["len_hist"], (cell[ended], t[ended]), 1)
        np.add.at(counts["episodes"], cell[ended], 1)
        fin = live & done[s]
        ep_count[fin] += 1
        ep_t[live & ~done[s]] += 1
        ep_t[fin] = 0
    return counts


def _bin_centres(world):
    w = _world(world)
    xc = w["wall_xmin"] + (np.arange(BX) + 0.5) * (w["wall_xmax"] - w["wall_xmin"]) / BX
    yc = w["wall_ymin"] + (np.arange(BY) + 0.5) * (w["wall_ymax"] - w["wall_ymin"]) / BY
    return xc, yc


def fingerprint_rows(counts, world=None):
    """The integer maps -> float64 (n_cells, len(FINGERPRINT_COLUMNS)), on the host; every positional statistic is taken over
    bin centres.  Per cell: the mean episode length (a length is t + 1 for an episode that ended at step-in-episode t); per
    team the shots per alive agent-step, the occupancy-weighted mean y and standard deviation of x, the in-episode deaths per
    alive agent-step; the share of guard occupancy in bins whose centre is within 2 * fort_dim of the door; the share of
    attacker occupancy with centre y > 0.  A cell without steps gives zeros, and so does a team that was never alive."""
    w = _world(world)
    xc, yc = _bin_centres(w)
    n_cells = np.asarray(counts["steps"]).shape[0]
    rows = np.zeros((n_cells, len(FINGERPRINT_COLUMNS)))
    near = np.hypot(xc[None, :] - w["door_x"], yc[:, None] - w["door_y"]) <= 2 * w["fort_dim"]      # (BY, BX)
    upper = np.broadcast_to((yc > 0)[:, None], (BY, BX))
    col = FINGERPRINT_COLUMNS.index
    for c in range(n_cells):
        if int(counts["steps"][c]) == 0:
            continue
        n_ep = float(counts["episodes"][c])
        if n_ep > 0:
            MT = np.asarray(counts["len_hist"]).shape[1]
            rows[c, 0] = float((np.asarray(counts["len_hist"][c], np.float64) * (np.arange(MT) + 1)).sum()) / n_ep
        for team, name in enumerate(("guard", "attacker")):
            occ = np.asarray(counts["occ"][c, team], np.float64)
            tot = occ.sum()
            if tot == 0:
                continue
            rows[c, col(name + "_shots_per_alive_step")] = float(np.asarray(counts["shots"][c, team]).sum()) / tot
            rows[c, col(name + "_deaths_per_alive_step")] = float(np.asarray(counts["deaths"][c, team]).sum()) / tot
            rows[c, col(name + "_mean_y")] = (occ.sum(1) * yc).sum() / tot
            mx = (occ.sum(0) * xc).sum() / tot
            rows[c, col(name + "_std_x")] = np.sqrt((occ.sum(0) * (xc - mx) ** 2).sum() / tot)
            if team == 0:
                rows[c, col("guard_share_near_door")] = occ[near].sum() / tot
            else:
                rows[c, col("attacker_share_upper_half")] = occ[upper].sum() / tot
    return rows


HEATMAP_SCALE, HEATMAP_GAP = 4, 2       # screen pixels per bin; grey pixels between two panels


def heatmap_image(counts_of_one_cell):
    """One cell's occ / shots / deaths (columns) of guards / attackers (rows) as a 2 x 3 grid of panels -> uint8 (H, W, 3),
    row 0 of the picture at the top (the bin row by = BY - 1, at wall_ymax).  A panel is scaled to its own maximum: a bin's
    level is round(255 * count / max); the guards' panels are green, the attackers' red, an empty panel is black."""
    S, P = HEATMAP_SCALE, HEATMAP_GAP
    img = np.full((2 * BY * S + P, 3 * BX * S + 2 * P, 3), 128, np.uint8)
    for team in range(2):
        for k, name in enumerate(("occ", "shots", "deaths")):
            m = np.asarray(counts_of_one_cell[name], np.float64)
            m = m.reshape((-1, 2, BY, BX))[0, team]                # with or without a leading axis of one cell
            top = m.max()
            level = np.rint(255.0 * m / top).astype(np.uint8) if top > 0 else np.zeros((BY, BX), np.uint8)
            level = np.repeat(np.repeat(level[::-1], S, 0), S, 1)
            panel = np.zeros((BY * S, BX * S, 3), np.uint8)
            panel[..., 1 if team == 0 else 0] = level
            y0, x0 = team * (BY * S + P), k * (BX * S + P)
            img[y0:y0 + BY * S, x0:x0 + BX * S] = panel
    return img


def write_heatmaps(path, counts_of_one_cell):
    """heatmap_image of one cell -> a PNG through PIL."""
    try:
        from PIL import Image
    except ImportError as exc:
        raise RuntimeError("write_heatmaps needs PIL (the Pillow package), which cannot be imported: %s; "
                           "the counts themselves are in behaviour.npz" % exc)
    Image.fromarray(heatmap_image(counts_of_one_cell), "RGB").save(path, format="PNG")


class BehaviourMaps(object):
    """BehaviourMaps(eng, env_cell, n_cells, episodes_per_env=0): the behaviour record of `eng` (a BatchedFortAttack with a
    bound storage) on the device.  begin() after the reset that starts a match (or between training rollouts): zeroes the
    record, ep_count = 0, ep_t = the world's time_step; chunk() after every chunk of storage.num_steps steps: one launch on
    fixed pointers, capturable in a graph; counts() -> the dict of int64 arrays, raw() the device buffer (n_cells, cell_words)
    of uint64 words held as int64.  episodes_per_env = 0: no quota.  `counts`: an own device int64 buffer of at least
    n_cells * cell_words elements (the record is its head)."""

    def __init__(self, eng, env_cell, n_cells, episodes_per_env=0, counts=None):
        import torch
        self.eng, self.n_cells, self.episodes_per_env = eng, int(n_cells), int(episodes_per_env)
        if not torch.is_tensor(env_cell):
            env_cell = torch.from_numpy(np.ascontiguousarray(env_cell, np.int32))
        self.env_cell = env_cell.to(eng.device, torch.int32).contiguous()
        if self.env_cell.numel() != eng.E:
            raise ValueError("BehaviourMaps: env_cell must hold one cell per env (%d), got %d" % (eng.E, self.env_cell.numel()))
        self.words = eng.behaviour_cell_words()
        n = max(self.n_cells, 0) * self.words
        if counts is None:
            counts = torch.zeros(max(n, 1), dtype=torch.int64, device=eng.device)
        if not (counts.is_cuda and counts.dtype == torch.int64 and counts.is_contiguous() and counts.numel() >= n):
            raise ValueError("BehaviourMaps: counts must be a contiguous device int64 tensor of >= %d elements" % n)
        self._buf = counts

    def begin(self):
        self.eng.behaviour_begin(self.env_cell, self.n_cells, self.episodes_per_env, self._buf)

    def chunk(self):
        self.eng.behaviour_chunk()

    def raw(self):
        return self._buf[:self.n_cells * self.words].view(self.n_cells, self.words)

    def counts(self):
        return unpack_counts(self.raw().cpu().numpy(), self.n_cells, self.eng.max_time_steps)

    def episode_counters(self):
        """(ep_count, ep_t): the per-env counters as numpy int32 (synchronises)."""
        return self.eng.behaviour_state()
