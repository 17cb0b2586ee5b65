"""GPU: cross-play evaluation -- the guard pool of the fused policy kernel (bit for bit the single-policy launches), the match
bookkeeping kernels against host bookkeeping from the CPU oracle, the CrossPlay evaluator end to end (eager and replayed
from a hipGraph), and shards adding up to the whole."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def fa():
    import emergent_multiagent_strategies_amd as m
    assert torch.cuda.is_available()
    m._lib.load()
    return m


def _policy(fa, n, m, seed):
    torch.manual_seed(seed)
    pol = fa.MPNN(num_agents=n, num_opp_agents=m, num_actions=8).cuda().eval()
    for p in pol.parameters():          # non-zero biases, larger logits than the 0.01-gain init gives
        if p.dim() == 1:
            p.data.uniform_(-0.3, 0.3)
        p.requires_grad_(False)
    pol.dist.linear.weight.data.mul_(3.0)
    return pol


def _obs(E, N, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    obs = torch.randn((E, N, 6), device="cuda", generator=g)
    obs[:, :, 0] = (torch.rand((E, N), device="cuda", generator=g) > 0.3).float()
    obs[:, :, 3] = obs[:, :, 3] * 3 + 4.7
    return obs.contiguous()


def _guard_ids(E):
    """Strategy counts 43 / 0 / 26 / 1 of 70 (scaled for other E): an unused strategy, a single env, several tiles with a
    partial last one; scattered over the handle."""
    n0, n2 = (43 * E) // 70, (26 * E) // 70
    ids = np.concatenate([np.zeros(n0), np.full(n2, 2), np.full(1, 3), np.zeros(E - n0 - n2 - 1)]).astype(np.int32)
    return ids[np.random.RandomState(E).permutation(E)]


# ---- 1. guard pool == single-policy launches ----------------------------------------------------------------------
@pytest.mark.parametrize("G,A,E", [(3, 3, 70), (2, 4, 70), (5, 5, 70), (3, 3, 3072)])
def test_guard_pool_equals_single_policy_launches_bit_for_bit(fa, G, A, E):
    """A row's arithmetic does not depend on its tile slot or its tile-mates (each MFMA output row reads only its own A row,
    attention stays inside the env's 16-lane group, the Philox key holds the global env index): no tolerance."""
    from emergent_multiagent_strategies_amd import mpnn_pack
    N, Kg, Ka = G + A, 4, 3
    guards = [_policy(fa, G, A, 100 + k) for k in range(Kg)]
    attackers = [_policy(fa, A, G, 200 + k) for k in range(Ka)]
    gpool = torch.stack([mpnn_pack.pack_policy(p) for p in guards]).contiguous()
    apool = torch.stack([mpnn_pack.pack_policy(p) for p in attackers]).contiguous()
    eng = fa.BatchedFortAttack(E, G, A, 20, env_offset=11)
    assert eng.policy_variant() == ("fa_policy_kernel<3, 8>" if E == 3072 else "fa_policy_kernel<2, 4>")
    gid_np = _guard_ids(E)
    if E == 70:
        assert np.bincount(gid_np, minlength=Kg).tolist() == [43, 0, 26, 1]
    gid = torch.from_numpy(gid_np).cuda()
    aid = torch.from_numpy(np.random.RandomState(7).randint(0, Ka, size=E).astype(np.int32)).cuda()
    obs = _obs(E, N, 3 * E + G)
    counter = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    gs = slice(0, G)
    for mode in ("sample", "deterministic", "value_only", "attn"):
        kw = dict(seed=77, counter=counter, step=3, pool=apool, env_strategy=aid,
                  deterministic=mode == "deterministic", value_only=mode == "value_only", return_attn=mode == "attn")
        got = eng.policy_act(obs, None, None, guard_pool=gpool, env_guard_strategy=gid, **kw)
        torch.cuda.synchronize()
        for g in range(Kg):
            ref = eng.policy_act(obs, gpool[g], None, **kw)
            sel = gid == g
            for k in range(3):
                if got[k] is None:
                    assert ref[k] is None and mode == "value_only"
                    continue
                assert torch.equal(got[k][sel][:, gs], ref[k][sel][:, gs]), (mode, g, k)     # g's envs: the guard rows
                assert torch.equal(got[k][:, G:], ref[k][:, G:]), (mode, g, k)               # attacker rows: every launch
            if mode == "attn":
                (tg, og), (ta, oa) = got[3]
                (rtg, rog), (rta, roa) = ref[3]
                assert torch.equal(tg[sel], rtg[sel]) and torch.equal(og[sel], rog[sel]), g
                assert torch.equal(ta, rta) and torch.equal(oa, roa), g
        if mode in ("sample", "deterministic"):      # ... and the log-probs are the env's strategy's (the module, 1e-4)
            value, act, lp = got
            with torch.no_grad():
                lp_all = torch.stack([p.evaluate_actions(obs[:, gs], obs[:, G:], act[:, gs].unsqueeze(-1))[1] for p in guards])
            want = lp_all[gid.long(), torch.arange(E, device="cuda")][..., 0]
            assert (want - lp[:, gs]).abs().max() < 1e-4, mode
            assert int(act.min()) >= 0 and int(act.max()) <= 7


def test_guard_pool_arguments_are_checked(fa):
    from emergent_multiagent_strategies_amd import mpnn_pack
    G, A, E = 3, 3, 8
    eng = fa.BatchedFortAttack(E, G, A, 20)
    w = mpnn_pack.pack_policy(_policy(fa, G, A, 1))
    obs = _obs(E, G + A, 1)
    ids = torch.zeros(E, dtype=torch.int32, device="cuda")
    with pytest.raises(fa.FaError, match="guard pool"):
        eng.policy_act(obs, None, w, guard_pool=w[None].expand(65, -1).contiguous(), env_guard_strategy=ids)
    io = eng._policy_io(None, w, 0, None, 0, False, False, None, None)
    io.guard_pool_size = 2                      # a set size with a NULL pool / NULL index array
    out = [torch.zeros((E, G + A), device="cuda") for _ in range(2)] + [torch.zeros((E, G + A), dtype=torch.int64, device="cuda")]
    io.obs, io.value, io.log_prob, io.action = obs.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr()
    import ctypes as C
    lib = fa._lib.load()
    assert lib.fa_policy_act(eng._h, C.byref(io), None) == -1 and b"guard pool" in lib.fa_last_error()
    io.guard_pool = w.data_ptr()
    assert lib.fa_policy_act(eng._h, C.byref(io), None) == -1 and b"guard pool" in lib.fa_last_error()


# ---- host bookkeeping from the oracle ----------------------------------------------------------------------------
class HostBook(object):
    """The reference's per-episode bookkeeping (test_fortattack_v2.py:88-101) on the host, from the oracle's per-step outputs:
    per env the list of finished episodes (result one-hot (3), alive at the end (N), return (N)) with the step they ended at."""

    def __init__(self, orc):
        self.orc, self.E, self.N = orc, orc.E, orc.N
        self.ep_rew = np.zeros((self.E, self.N))
        self.episodes = [[] for _ in range(self.E)]
        self.t = 0

    def step(self, actions):
        """One step of every env with auto-reset semantics; returns (ref, obs_next): the oracle's outputs and the observation
        row that follows (the reset observation where the episode ended)."""
        orc = self.orc
        ref = orc.step(actions, auto_reset=False)
        self.ep_rew += ref["reward"] * ref["alive_before"]
        d = ref["done"].astype(bool)
        obs_next = ref["obs"].copy()
        if d.any():
            gr = orc.get_state()["game_result"]
            for e in np.nonzero(d)[0]:
                self.episodes[e].append((self.t, gr[e].astype(np.int64).copy(), ref["obs"][e, :, 0].astype(np.int64).copy(),
                                         self.ep_rew[e].copy()))
                self.ep_rew[e] = 0
            obs_next[d] = orc.reset(mask=d)[d]
        self.t += 1
        return ref, obs_next

    def raw(self, cell, n_cells, quota, upto=None):
        """(n_cells, 5 + 2N) sums of the first `quota` episodes of every env that finished them within the first `upto` steps;
        also the sum of |terms| of the reward columns (for the summation-order bound)."""
        N = self.N
        raw, mag = np.zeros((n_cells, 5 + 2 * N)), np.zeros((n_cells, N))
        upto = self.t if upto is None else upto
        for c in range(n_cells):
            envs = [e for e in range(self.E) if cell[e] == c and len(self.episodes[e]) >= quota
                    and self.episodes[e][quota - 1][0] < upto]
            rew = np.zeros((len(envs), N))
            for k, e in enumerate(envs):
                eps = self.episodes[e][:quota]
                raw[c, 0] += 1
                raw[c, 1] += quota
                raw[c, 2:5] += sum(ep[1] for ep in eps)
                raw[c, 5:5 + N] += sum(ep[2] for ep in eps)
                acc = np.zeros(N)
                for ep in eps:                       # the device adds the episodes' returns in this order
                    acc = acc + ep[3]
                rew[k] = acc
            raw[c, 5 + N:] = rew.sum(0) if envs else 0.0
            mag[c] = np.abs(rew).sum(0) if envs else 0.0
        return raw, mag


def _assert_raw(got, want, mag, E, N):
    assert np.array_equal(got[:, :5 + N], want[:, :5 + N])                      # integer columns
    err = np.abs(got[:, 5 + N:] - want[:, 5 + N:])
    print("reward sums: max |device - numpy| = %.3e, bound min %.3e" % (err.max(), (E * EPS * mag).min()))
    assert (err <= E * EPS * mag).all(), (err.max(), (E * EPS * mag))


# ---- 2. latch and table ------------------------------------------------------------------------------------------
E2, G2, A2, MAXT2, QUOTA2 = 37, 2, 3, 5, 3
CELL2 = np.concatenate([np.zeros(20), np.full(12, 2), np.full(5, 3)]).astype(np.int32)[np.random.RandomState(2).permutation(E2)]


def _drive(fa, steps, latch=lambda t: True, seed=31):
    """Fresh handle + fresh oracle, the same random actions to both, one step per launch, match_latch after step t iff latch(t)."""
    from fa_oracle import OracleEnv
    N = G2 + A2
    eng = fa.BatchedFortAttack(E2, G2, A2, MAXT2, base_seed=seed)
    book = HostBook(OracleEnv(E2, G2, A2, MAXT2, base_seed=seed))
    eng.match_begin(torch.from_numpy(CELL2).cuda(), 4, QUOTA2)
    eng.reset(), book.orc.reset()
    rng = np.random.RandomState(seed)
    for t in range(steps):
        a = np.where(rng.rand(E2, N) < 0.3, 7, rng.randint(0, 8, size=(E2, N)))
        eng.step(torch.from_numpy(a).cuda(), auto_reset=True, want=("done",))
        if latch(t):
            eng.match_latch()
        book.step(a)
    return eng, book


def test_match_latch_and_table_against_host_bookkeeping(fa):
    N = G2 + A2
    eng, book = _drive(fa, 15)
    raw, remaining = eng.match_table()
    got = raw.cpu().numpy()
    want, mag = book.raw(CELL2, 4, QUOTA2)
    assert got.shape == (4, 5 + 2 * N) and remaining == 0
    assert got[:, 0].tolist() == [20, 0, 12, 5] and (got[1] == 0).all() and (got[:, 1] == QUOTA2 * got[:, 0]).all()
    _assert_raw(got, want, mag, E2, N)
    # latched numbers never change again: five more steps and latches, the same bits
    rng = np.random.RandomState(5)
    for t in range(5):
        a = np.where(rng.rand(E2, N) < 0.3, 7, rng.randint(0, 8, size=(E2, N)))
        eng.step(torch.from_numpy(a).cuda(), auto_reset=True, want=("done",))
        eng.match_latch()
    raw2, remaining2 = eng.match_table()
    assert remaining2 == 0 and np.array_equal(raw2.cpu().numpy().view(np.int64), got.view(np.int64))
    # ... and two table calls give the same bits
    raw3, _ = eng.match_table()
    assert torch.equal(raw3, raw2)


def test_match_table_counts_only_latched_envs(fa):
    N = G2 + A2
    eng, book = _drive(fa, 4)
    raw, remaining = eng.match_table()
    want, mag = book.raw(CELL2, 4, QUOTA2)
    assert remaining == E2 - int(want[:, 0].sum()) and remaining > 0
    _assert_raw(raw.cpu().numpy(), want, mag, E2, N)


def test_match_table_refuses_skipped_latches(fa):
    # two episodes latched step by step, then 2 * max_time_steps steps without a latch: at least two more episodes end, beyond
    # the quota of three
    eng, _ = _drive(fa, 4 * MAXT2, latch=lambda t: t < 2 * MAXT2)
    eng.match_latch()
    with pytest.raises(fa.FaError, match=r"\(-3\).*beyond episodes_per_env"):
        eng.match_table()
    # without that last latch the table finds them itself
    eng, _ = _drive(fa, 4 * MAXT2, latch=lambda t: t < 2 * MAXT2)
    with pytest.raises(fa.FaError, match=r"\(-3\)"):
        eng.match_table()


def test_match_calls_need_counters_and_a_begin(fa):
    eng = fa.BatchedFortAttack(8, 2, 3, 5, track_counters=False)
    with pytest.raises(fa.FaError, match="track_counters"):
        eng.match_begin(torch.zeros(8, dtype=torch.int32, device="cuda"), 1, 1)
    eng = fa.BatchedFortAttack(8, 2, 3, 5)
    with pytest.raises(fa.FaError, match="fa_match_begin"):
        eng.match_latch()


# ---- 3. / 4. the evaluator ---------------------------------------------------------------------------------------
E3, G3, A3, MAXT3, QUOTA3, SEED3 = 60, 3, 3, 8, 2, 13
_RUNS = {}


def _pools(fa):
    if "pools" not in _RUNS:
        _RUNS["pools"] = ([_policy(fa, G3, A3, 300 + k) for k in range(2)], [_policy(fa, A3, G3, 400 + k) for k in range(3)])
    return _RUNS["pools"]


def _crossplay(fa, E, env_offset, use_graph):
    guards, attackers = _pools(fa)
    eng = fa.BatchedFortAttack(E, G3, A3, MAXT3, base_seed=SEED3, env_offset=env_offset)
    return fa.CrossPlay(eng, guards, attackers, QUOTA3, sample_seed=9, use_graph=use_graph)


def _run_checked(fa, use_graph):
    """One whole evaluation driven chunk by chunk, every chunk's storage checked; -> (device raw, host raw, sum |terms|)."""
    if use_graph in _RUNS:
        return _RUNS[use_graph]
    from fa_oracle import OracleEnv
    guards, attackers = _pools(fa)
    N, G = G3 + A3, G3
    cp = _crossplay(fa, E3, 0, use_graph)
    assert cp.T == MAXT3 and cp.n_cells == 6
    cell, gid, aid = fa.crossplay_cells(E3, 0, 2, 3)
    assert np.array_equal(cp.cell.cpu().numpy(), cell)
    book = HostBook(OracleEnv(E3, G3, A3, MAXT3, base_seed=SEED3))
    cp.begin()
    obs_next = book.orc.reset()
    gsl, asl = slice(0, G), slice(G, N)
    ar = torch.arange(E3, device="cuda")
    remaining = E3
    while remaining:
        assert cp.steps_run < 16                                            # every episode ends at its timeout
        if cp.steps_run:
            cp.eng.after_update()
        remaining = cp.run_chunk()
        st = cp.storage
        obs, rew, msk, done, acts = [getattr(st, k).cpu().numpy() for k in ("obs", "rewards", "masks", "done", "actions")]
        assert np.array_equal(obs[0], obs_next.astype(np.float32))
        for s in range(cp.T):                                               # env rows: the oracle driven by the stored actions
            ref, obs_next = book.step(acts[s, :, :, 0])
            assert np.array_equal(done[s], ref["done"]), s
            assert np.array_equal(obs[s + 1], obs_next.astype(np.float32)), s
            assert np.array_equal(rew[s, :, :, 0], ref["reward"].astype(np.float32)), s
            want_mask = np.where(ref["done"][:, None] != 0, 1, ref["alive_before"]).astype(np.float32)
            assert np.array_equal(msk[s + 1, :, :, 0], want_mask), s
        with torch.no_grad():                                               # log-probs: the cell's two policies
            for s in range(cp.T):
                o = st.obs[s]
                lg = torch.stack([p.evaluate_actions(o[:, gsl], o[:, asl], st.actions[s, :, gsl])[1] for p in guards])
                la = torch.stack([p.evaluate_actions(o[:, asl], o[:, gsl], st.actions[s, :, asl])[1] for p in attackers])
                assert (lg[cp.guard_id.long(), ar] - st.action_log_probs[s, :, gsl]).abs().max() < 1e-4, s
                assert (la[cp.attacker_id.long(), ar] - st.action_log_probs[s, :, asl]).abs().max() < 1e-4, s
    assert remaining == 0 and cp.steps_run <= 16
    got = cp.raw().cpu().numpy().copy()
    want, mag = book.raw(cell, 6, QUOTA3)
    assert (got[:, 0] == 10).all() and (got[:, 1] == 20).all()
    _assert_raw(got, want, mag, E3, N)
    table = cp.table()
    assert table.shape == (2, 3, 8) and np.array_equal(table.reshape(6, 8), fa.crossplay_rows(got, G))
    assert np.allclose(table[..., 2], 1.0 - table[..., 3])
    _RUNS[use_graph] = (got, want, mag)
    return _RUNS[use_graph]


@pytest.mark.parametrize("use_graph", [False, True])
def test_crossplay_end_to_end(fa, use_graph):
    got = _run_checked(fa, use_graph)[0]
    eager = _run_checked(fa, False)[0]                                      # eager and graph runs: identical bits
    assert np.array_equal(got.view(np.int64), eager.view(np.int64))


def test_crossplay_run_and_shards_add_up(fa):
    N = G3 + A3
    eager, _, mag = _run_checked(fa, False)
    whole = _crossplay(fa, E3, 0, False).run()
    assert whole.remaining == 0 and whole.steps_run <= 16
    got = whole.raw().cpu().numpy()
    assert np.array_equal(got.view(np.int64), eager.view(np.int64))        # run() == the chunks driven by hand
    parts = [_crossplay(fa, 30, off, False).run().raw().cpu().numpy() for off in (0, 30)]
    total = parts[0] + parts[1]
    assert np.array_equal(total[:, :5 + N], got[:, :5 + N])
    err = np.abs(total[:, 5 + N:] - got[:, 5 + N:])
    print("shards: max |sum of parts - whole| = %.3e" % err.max())
    assert (err <= E3 * EPS * mag).all()
