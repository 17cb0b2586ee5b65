"""Cross-play evaluation: a series of guard checkpoints against every attacker strategy, all match-ups at once.

The reference's result scripts (test_fortattack_v2.py:56-124, test_fortattack_v2_gen_plot_data.py:61-141) load one guard
checkpoint after the other, play each against every published attacker strategy for a fixed number of episodes, one env
at a time, and emit one row per match-up.  Here one handle plays the whole ``guard checkpoints x attacker strategies``
matrix: every env is assigned a (guard, attacker) cell, the fused policy kernel runs each team's envs grouped by that
team's strategy (fa_policy_io.guard_pool / attacker_pool), every env contributes exactly ``episodes_per_env`` episodes
(fa_match_begin / fa_match_latch) and the per-cell sums are built on the device (fa_match_table).
"""
import numpy as np
import torch

from . import mpnn_pack
from .behaviour import BehaviourMaps, fingerprint_rows
from .learner import _capture_mode, _warm_state
from .mpnn import MPNN
from .storage import JointRolloutStorage


def crossplay_cells(E, env_offset, n_guard, n_attacker):
    """(cell, guard_id, attacker_id), each (E,) int32: env e of a handle whose first env has the global index `env_offset`
    plays cell (env_offset + e) % (n_guard * n_attacker) -- a function of the GLOBAL env index, so shards of a larger
    batch get the assignment the one large handle has."""
    cell = ((int(env_offset) + np.arange(int(E), dtype=np.int64)) % (int(n_guard) * int(n_attacker))).astype(np.int32)
    return cell, (cell // int(n_attacker)).astype(np.int32), (cell % int(n_attacker)).astype(np.int32)


def crossplay_rows(raw, G):
    """Raw per-cell sums (n_cells, 5 + 2N) [latched envs, episodes, result_count[3], alive_at_end[N],
    episode_reward_sum[N]] -> (n_cells, 8), the reference's row per match-up (test_fortattack_v2.py:95-101) as means over
    the cell's episodes: [attackers all dead, timeout, guards win, fort reached, guards alive, attackers alive, mean
    guard return, mean attacker return].  A cell without episodes gives zeros."""
    raw = np.asarray(raw, np.float64)
    N = (raw.shape[1] - 5) // 2
    rows = np.zeros((raw.shape[0], 8))
    for c in range(raw.shape[0]):
        n_ep = raw[c, 1]
        if n_ep <= 0:
            continue
        rc = raw[c, 2:5] / n_ep
        alive = raw[c, 5:5 + N] / n_ep
        rew = raw[c, 5 + N:5 + 2 * N] / n_ep
        rows[c] = [rc[0], rc[1], rc[0] + rc[1], rc[2], alive[:G].sum(), alive[G:].sum(), rew[:G].mean(), rew[G:].mean()]
    return rows


def _load_policy(src, team, n_own, n_opp, device):
    """A path, a checkpoint dict ({"models": [...]}), a state_dict or an MPNN module -> a frozen MPNN of that team on `device`
    (guards from models[0], attackers from models[-1]: learner.py:245-249, :137-139)."""
    if isinstance(src, MPNN):
        pol = src
    else:
        if isinstance(src, str):
            src = torch.load(src, map_location="cpu", weights_only=False)
        sd = src["models"][0 if team == 0 else -1] if isinstance(src, dict) and "models" in src else src
        pol = MPNN(num_agents=n_own, num_opp_agents=n_opp, hidden_dim=mpnn_pack.HIDDEN, num_actions=8)
        try:
            pol.load_state_dict(sd)
        except RuntimeError as exc:
            raise ValueError("CrossPlay runs on the fused policy kernel only: hidden_dim = 128, 6 inputs, 8 actions, teams "
                             "of <= 8 (there is no PyTorch fallback for a guard pool); this checkpoint does not fit: %s" % exc)
    if not mpnn_pack.supported(pol) or pol.num_agents != n_own or pol.num_opp_agents != n_opp:
        raise ValueError("CrossPlay runs on the fused policy kernel only: hidden_dim = 128, 6 inputs, 8 actions, teams of <= 8 "
                         "and the handle's team sizes (there is no PyTorch fallback for a guard pool)")
    pol = pol.to(device).eval()
    for p in pol.parameters():
        p.requires_grad_(False)
    return pol


class CrossPlay(object):
    """CrossPlay(eng, guard_policies, attacker_policies, episodes_per_env): run() plays episodes_per_env episodes on every env
    of `eng` (a BatchedFortAttack with track_counters), env e in cell crossplay_cells(...)[e]; table() is the
    (n_guard, n_attacker, 8) matrix of reference rows, raw() the device sums they come from (add the raw() of shards or
    ranks to merge them).  Sampling (deterministic=False) is the reference's evaluation mode: Learner.act samples.
    recorder: a record.EpisodeRecorder over some of the handle's envs (record_envs() picks them; it may also be assigned to
    `.recorder` before begin()): every step's frames are drawn on the device -- inside the chunk's graph when use_graph is
    set -- and brought to the host once per chunk.  What is played does not depend on it.
    behaviour: keep the behaviour record of every match-up (behaviour.BehaviourMaps) over the episodes that count for the
    match: one more launch at the end of every chunk -- the last node of the chunk's graph -- over the storage the chunk
    left; behaviour_counts() / fingerprints() return it.  What is played, raw() and the storage do not depend on it."""

    def __init__(self, eng, guard_policies, attacker_policies, episodes_per_env, num_steps=None, deterministic=False,
                 sample_seed=0, use_graph=False, recorder=None, behaviour=False):
        self.eng, self.device = eng, eng.device
        self.E, self.G, self.A, self.N = eng.E, eng.G, eng.A, eng.N
        if not eng.cfg.track_counters:
            raise ValueError("CrossPlay needs a handle created with track_counters=True")
        self.guards = [_load_policy(p, 0, self.G, self.A, self.device) for p in guard_policies]
        self.attackers = [_load_policy(p, 1, self.A, self.G, self.device) for p in attacker_policies]
        self.n_guard, self.n_attacker = len(self.guards), len(self.attackers)
        if not (1 <= self.n_guard <= 64 and 1 <= self.n_attacker <= 64):
            raise ValueError("CrossPlay: 1..64 guard policies and 1..64 attacker policies")
        self.n_cells = self.n_guard * self.n_attacker
        self.episodes_per_env = int(episodes_per_env)
        self.T = int(num_steps) if num_steps is not None else int(eng.max_time_steps)
        self.deterministic, self.sample_seed, self.use_graph = bool(deterministic), int(sample_seed), bool(use_graph)
        # both pools, packed once
        self.guard_pool = torch.stack([mpnn_pack.pack_policy(p) for p in self.guards]).contiguous()
        self.attacker_pool = torch.stack([mpnn_pack.pack_policy(p) for p in self.attackers]).contiguous()
        cell, gid, aid = crossplay_cells(self.E, eng.cfg.env_offset, self.n_guard, self.n_attacker)
        dev = lambda a: torch.from_numpy(a).to(self.device)
        self.cell, self.guard_id, self.attacker_id = dev(cell), dev(gid), dev(aid)
        self.storage = JointRolloutStorage(self.T, self.E, self.N, device=self.device)
        eng.bind_storage(self.storage)
        self._counter = torch.zeros(1, dtype=torch.int64, device=self.device)   # part of the sampling key: one per chunk
        self._raw = torch.zeros((self.n_cells, 5 + 2 * self.N), dtype=torch.float64, device=self.device)
        self._graph = None
        self.steps_run = 0
        self.remaining = self.E
        self.on_chunk = None        # optional callable(self) after every chunk, before after_update (the storage is whole)
        self.recorder = recorder
        self._attn_out = None       # the step's attention maps, exported only for a recorder that draws them
        self.behaviour = BehaviourMaps(eng, self.cell, self.n_cells, self.episodes_per_env) if behaviour else None

    def record_envs(self, per_cell=1):
        """The first `per_cell` env indices of every match-up cell, in cell order (a cell with fewer envs gives what it has):
        the envs an EpisodeRecorder of this evaluation would watch."""
        cell = self.cell.cpu().numpy()
        return np.concatenate([np.nonzero(cell == c)[0][:int(per_cell)] for c in range(self.n_cells)]).astype(np.int64)

    # ---- one chunk -----------------------------------------------------------------------------------------------
    def _step(self, s):
        rec = self.recorder
        attn_out = self._attn_out if rec is not None else None
        self.eng.collect_act(s, None, None, self.sample_seed, self._counter, deterministic=self.deterministic,
                             pool=self.attacker_pool, env_strategy=self.attacker_id,
                             guard_pool=self.guard_pool, env_guard_strategy=self.guard_id, attn_out=attn_out)
        self.eng.collect_step(s, auto_reset=True)
        self.eng.match_latch()
        if rec is not None:
            rec.capture(s, self.storage, attn_out)

    def _capture(self):
        """ONE hipGraph for a chunk: T x (act with both pools, env step, latch[, the recorder's frames])[, the behaviour pass].
        Every launch argument is a fixed pointer."""
        if self.eng.max_time_steps < 8:
            raise ValueError("use_graph needs max_time_steps >= 8 (the warm-up step must not end an episode)")
        _warm_state(self.eng, self.storage, self.G, self.A)
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._step(0)               # code objects loaded before the capture
            if self.behaviour is not None:
                self.behaviour.chunk()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode=_capture_mode()):
            for s in range(self.T):
                self._step(s)
            if self.behaviour is not None:
                self.behaviour.chunk()
        # the warm-up step set prevDist; it survives resets in the reference, so put back "None"
        self.eng.set_state(dict(prev_dist=np.full((self.E, self.N), np.nan)))
        return g

    def begin(self):
        """fa_match_begin + a reset of every env (obs[0] <- the reset observations); with a recorder, its reset frame.  (run()
        also hands every chunk to the recorder; a caller that drives run_chunk() itself calls recorder.end_chunk(storage).)"""
        rec = self.recorder
        if rec is not None and rec.T != self.T:
            raise ValueError("CrossPlay: the recorder's num_steps (%d) must be the chunk length (%d)" % (rec.T, self.T))
        if rec is not None and rec.viz_attn and self._attn_out is None:
            self._attn_out = self.eng.new_attn_out()        # fixed buffers, allocated before any capture
        self.eng.match_begin(self.cell, self.n_cells, self.episodes_per_env)
        if self.use_graph and self._graph is None:
            if self.behaviour is not None:
                self.behaviour.begin()                      # the warm-up launch needs a record; begun again below
            self._graph = self._capture()
            self.eng.match_begin(self.cell, self.n_cells, self.episodes_per_env)   # the warm-up step is no part of the match
        self.eng.collect_reset()
        if self.behaviour is not None:
            self.behaviour.begin()                          # after the reset: ep_t starts from the world's time_step
        if rec is not None:
            rec.capture_reset()
        self.steps_run, self.remaining = 0, self.E

    def run_chunk(self):
        """num_steps x (collect_act with both pools -> collect_step(auto_reset) -> match_latch)[, the behaviour pass];
        returns `remaining`, the number of envs still short of their quota (read once, here)."""
        self._counter.add_(1)
        if self._graph is not None:
            self._graph.replay()
        else:
            for s in range(self.T):
                self._step(s)
            if self.behaviour is not None:
                self.behaviour.chunk()
        self.steps_run += self.T
        _, self.remaining = self.eng.match_table(self._raw)
        return self.remaining

    def run(self):
        """begin, then chunks with after_update() between them until every env has its episodes.  Every episode ends at its
        timeout at the latest, so episodes_per_env * max_time_steps steps always suffice: envs remaining after that are a bug."""
        self.begin()
        limit = self.episodes_per_env * self.eng.max_time_steps
        while True:
            rem = self.run_chunk()
            if self.recorder is not None:
                self.recorder.end_chunk(self.storage)
            if self.on_chunk is not None:
                self.on_chunk(self)
            if rem == 0:
                return self
            if self.steps_run >= limit:
                raise RuntimeError("CrossPlay: %d envs have not finished %d episodes after %d steps (max_time_steps = %d)"
                                   % (rem, self.episodes_per_env, self.steps_run, self.eng.max_time_steps))
            self.eng.after_update()

    # ---- results -------------------------------------------------------------------------------------------------
    def raw(self):
        """(n_cells, 5 + 2N) float64 device sums over the latched envs of every cell (fa_match_table)."""
        raw, self.remaining = self.eng.match_table(self._raw)
        return raw

    def table(self):
        """(n_guard, n_attacker, 8): the reference's row for every match-up (crossplay_rows)."""
        return crossplay_rows(self.raw().cpu().numpy(), self.G).reshape(self.n_guard, self.n_attacker, 8)

    def behaviour_counts(self):
        """The behaviour record (behaviour.BehaviourMaps.counts()): a dict of int64 arrays with a leading n_cells axis."""
        if self.behaviour is None:
            raise ValueError("CrossPlay: created without behaviour=True")
        return self.behaviour.counts()

    def fingerprints(self):
        """(n_guard, n_attacker, len(behaviour.FINGERPRINT_COLUMNS)): behaviour.fingerprint_rows of every match-up."""
        rows = fingerprint_rows(self.behaviour_counts(), self.eng.cfg.world)
        return rows.reshape(self.n_guard, self.n_attacker, rows.shape[1])
