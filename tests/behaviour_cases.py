"""Shared by test_behaviour_cpu.py and test_gpu_behaviour.py: a start state that brings the teams within laser range, an
independently structured restatement of the behaviour record (per env, per episode, dict counters), the hand-made edge rows
with their hand-derived expectations, and the non-triviality conditions both tests assert."""
import collections

import numpy as np

BX, BY = 40, 32


def close_state(E, G, A, seed):
    """Teams on two lines 0.3 apart, facing each other (guards look down, attackers up): a laser (shoot_rad 0.8, window
    pi / 4) hits from the first step on; the last agent of either team stands at x = 0.3, opposite the other team's last.  In
    every third env all attackers but the last are dead already: its episode can end early even against one guard."""
    rng = np.random.RandomState(seed)
    N = G + A
    x = np.concatenate([np.linspace(-0.3, 0.3, G) if G > 1 else np.full(1, 0.3), np.linspace(-0.3, 0.3, A) if A > 1 else np.full(1, 0.3)])
    pos_x = x[None, :] + rng.uniform(-0.04, 0.04, size=(E, N))
    pos_y = np.concatenate([np.full(G, 0.15), np.full(A, -0.15)])[None, :] + rng.uniform(-0.04, 0.04, size=(E, N))
    ang = np.tile(np.concatenate([np.full(G, 3 * np.pi / 2), np.full(A, np.pi / 2)])[None, :], (E, 1))
    alive = np.ones((E, N), np.uint8)
    alive[::3, G:N - 1] = 0
    return dict(pos_x=pos_x, pos_y=pos_y, vel_x=np.zeros((E, N)), vel_y=np.zeros((E, N)), ang=ang,
                prev_dist=np.full((E, N), np.nan), alive=alive, time_step=np.zeros(E, np.int32))


def state_obs(s):
    """The observation rows [alive, x, y, ang, vx, vy] of a state dict, float32."""
    return np.stack([s["alive"].astype(np.float64), s["pos_x"], s["pos_y"], s["ang"], s["vel_x"], s["vel_y"]], -1).astype(np.float32)


def random_actions(rng, shape):
    """Uniform actions with the laser (7) three times in ten."""
    return np.where(rng.rand(*shape) < 0.3, 7, rng.randint(0, 8, size=shape)).astype(np.int64)


def _bin(v, v0, scale, n):
    d = np.float32(np.float32(v) - np.float32(v0))
    f = float(np.floor(np.float32(d * np.float32(scale))))
    return int(min(max(f, 0.0), float(n - 1)))


def loop_reference(obs, actions, done, cell, ep_count, ep_t, n_cells, G, MT, quota, walls=(-1.0, 1.0, -0.8, 0.8)):
    """The record of one chunk, env by env and episode by episode, into a Counter keyed (section, cell, ...); ep_count / ep_t
    (lists or arrays) are advanced in place.  Written from the prose of the definition, not from the package's restatement."""
    T, E, N = obs.shape[0] - 1, obs.shape[1], obs.shape[2]
    actions = np.asarray(actions).reshape(T, E, N)
    x0, sx = np.float32(walls[0]), np.float32(BX / (walls[1] - walls[0]))
    y0, sy = np.float32(walls[2]), np.float32(BY / (walls[3] - walls[2]))
    cnt = collections.Counter()
    for e in range(E):
        c = int(cell[e])
        tabled = 0 <= c < n_cells
        s = 0
        while s < T:
            if quota > 0 and ep_count[e] >= quota:
                break
            ends = np.nonzero(done[s:, e])[0]                      # the episode in flight: rows s .. end of this chunk
            finished = len(ends) > 0
            end = s + int(ends[0]) if finished else T - 1
            for u in range(s, end + 1):
                t = min(int(ep_t[e]) + (u - s), MT - 1)
                if not tabled:
                    continue
                cnt["steps", c] += 1
                for i in range(N):
                    if obs[u, e, i, 0] == 0:
                        continue
                    team = 0 if i < G else 1
                    bx, by = _bin(obs[u, e, i, 1], x0, sx, BX), _bin(obs[u, e, i, 2], y0, sy, BY)
                    cnt["occ", c, team, by, bx] += 1
                    cnt["alive_t", c, team, t] += 1
                    if actions[u, e, i] == 7:
                        cnt["shots", c, team, by, bx] += 1
                    if u != end or not finished:                   # not the step that ended the episode
                        if obs[u + 1, e, i, 0] == 0:
                            cnt["deaths", c, team, by, bx] += 1
            if finished:
                if tabled:
                    cnt["len_hist", c, min(int(ep_t[e]) + (end - s), MT - 1)] += 1
                    cnt["episodes", c] += 1
                ep_count[e] += 1
                ep_t[e] = 0
            else:
                ep_t[e] += end + 1 - s
            s = end + 1
    return cnt


def counter_to_counts(cnt, n_cells, MT):
    shapes = dict(steps=(), episodes=(), len_hist=(MT,), alive_t=(2, MT), occ=(2, BY, BX), shots=(2, BY, BX), deaths=(2, BY, BX))
    out = {k: np.zeros((n_cells,) + s, np.int64) for k, s in shapes.items()}
    for key, v in cnt.items():
        out[key[0]][key[1:]] = v
    return out


def assert_counts_equal(got, want):
    for k in ("steps", "episodes", "len_hist", "alive_t", "occ", "shots", "deaths"):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == np.int64, k
        assert np.array_equal(g, w), (k, np.argwhere(g != w)[:5])


def assert_not_trivial(counts, MT, quota, history):
    """What makes a comparison worth its name: every map has counts, an episode ended before its timeout, and (with a quota)
    an env reached it in the middle of a chunk, so that the rest of its rows had to be cut.  history: per chunk (ep_count
    before, ep_count after, done (T, E))."""
    for k in ("occ", "shots", "deaths"):
        assert counts[k].sum() > 0, k
    assert counts["len_hist"][:, :MT - 1].sum() > 0                # ... an episode shorter than max_time_steps
    if quota > 0:
        mid = []
        for before, after, done in history:
            reached = (np.asarray(before) < quota) & (np.asarray(after) >= quota)
            mid += [e for e in np.nonzero(reached)[0]
                    if np.nonzero(done[:, e])[0][quota - 1 - int(before[e])] < done.shape[0] - 1]
        assert mid, "no env reached its quota mid-chunk"


# ---- hand-made rows: 1 guard + 1 attacker, T = 1, max_time_steps = 8, two cells, no quota ---------------------------------
EDGE_G, EDGE_A, EDGE_MT, EDGE_CELLS = 1, 1, 8, 2


def edge_case():
    """-> (obs (2, 7, 2, 6), actions (1, 7, 2), done (1, 7), cell (7), ep_t0 (7), want: {(section, cell, ...): count},
    want_ep_count (7), want_ep_t (7)).  The bins are derived by hand from the float32 contract (x0 = -1, sx = 20, y0 =
    float32(-0.8), sy = 20):
      x =  0.25 -> (1.25) * 20 = 25 exactly, an edge: bin 25;  x = -0.5 -> 10;  x = -0.0 and 0.0 -> 20
      x = nextafter(0.25, -inf) in float32: x - x0 rounds to 1.25 (the spacing above 1 is 2^-23): bin 25 as well
      x = +-1 (on the walls) -> 0 and 40 -> clamped 39;  x = 1.5, -1.2 (beyond) -> clamped 39, 0
      y = float32(-0.8) -> 0;  y = float32(0.8): 0.8f + 0.8f = 1.6f, * 20 rounds to 32.0 -> clamped 31;  y = +-1 -> 31, 0
      y = 0.0 and -0.0: 0.8f * 20 = 16.0000002 -> rounds to 16.0: bin 16;  y = float32(0.2): 0.2f + 0.8f rounds to 1.0: bin 20."""
    f = np.float32
    just_below = np.nextafter(f(0.25), f(-np.inf))
    # per env: (guard alive, x, y, action), (attacker alive, x, y, action), done, (guard, attacker) alive in the next row, cell, ep_t
    envs = [
        ((1, 0.25, 0.0, 7), (1, -0.5, -0.8, 0), 0, (1, 0), 0, 0),        # a guard's shot on an edge; the attacker dies
        ((1, 1.0, 0.8, 3), (1, -1.0, -0.8, 7), 1, (1, 0), 1, 2),         # on all four walls; a death on a done step: not counted
        ((0, 0.0, 0.0, 7), (1, -1.2, -1.0, 1), 0, (0, 1), 0, 1),         # a dead agent whose action is 7: not counted; beyond two walls
        ((1, 1.5, 1.0, 0), (1, -0.0, -0.0, 0), 0, (1, 1), 1, 100),       # beyond the other two; -0.0; ep_t beyond max_time_steps
        ((1, 0.1, 0.1, 7), (1, 0.2, 0.2, 7), 0, (0, 0), -1, 3),          # a cell below the range: counted nowhere
        ((1, 0.1, 0.1, 7), (1, 0.2, 0.2, 7), 1, (1, 1), EDGE_CELLS, 3),  # a cell above the range, and its episode ends
        ((1, just_below, 0.2, 0), (0, 0.3, 0.3, 0), 0, (1, 0), 0, 5),    # a hair below an edge; the attacker is dead already
    ]
    E = len(envs)
    obs = np.zeros((2, E, 2, 6), np.float32)
    actions = np.zeros((1, E, 2), np.int64)
    done = np.zeros((1, E), np.uint8)
    cell = np.zeros(E, np.int32)
    ep_t0 = np.zeros(E, np.int32)
    for e, (g, a, d, nxt, c, t0) in enumerate(envs):
        for i, (alive, x, y, act) in enumerate((g, a)):
            obs[0, e, i, :3] = (alive, x, y)
            obs[0, e, i, 3] = 1.0
            obs[1, e, i] = (nxt[i], 0.5, 0.5, 1.0, 0.0, 0.0)
            actions[0, e, i] = act
        done[0, e], cell[e], ep_t0[e] = d, c, t0
    want = {
        ("steps", 0): 3, ("steps", 1): 2, ("episodes", 1): 1, ("len_hist", 1, 2): 1,
        # env 0
        ("occ", 0, 0, 16, 25): 1, ("shots", 0, 0, 16, 25): 1, ("occ", 0, 1, 0, 10): 1, ("deaths", 0, 1, 0, 10): 1,
        ("alive_t", 0, 0, 0): 1, ("alive_t", 0, 1, 0): 1,
        # env 1
        ("occ", 1, 0, 31, 39): 2, ("occ", 1, 1, 0, 0): 1, ("shots", 1, 1, 0, 0): 1, ("alive_t", 1, 0, 2): 1, ("alive_t", 1, 1, 2): 1,
        # env 2 (the attacker only; its bin (0, 0) of cell 0)
        ("occ", 0, 1, 0, 0): 1, ("alive_t", 0, 1, 1): 1,
        # env 3: the guard shares bin (31, 39) of cell 1 with env 1's (counted above), t clamps to 7
        ("occ", 1, 1, 16, 20): 1, ("alive_t", 1, 0, 7): 1, ("alive_t", 1, 1, 7): 1,
        # env 6
        ("occ", 0, 0, 20, 25): 1, ("alive_t", 0, 0, 5): 1,
    }
    want_ep_count = np.array([0, 1, 0, 0, 0, 1, 0], np.int32)
    want_ep_t = np.array([1, 0, 2, 101, 4, 0, 6], np.int32)
    return obs, actions, done, cell, ep_t0, want, want_ep_count, want_ep_t
