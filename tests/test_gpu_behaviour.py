"""GPU: the behaviour pass (csrc/fa_behaviour.hip) against its numpy restatement on storages the collector filled, word for
word including what lies behind the record; the hand-made edge rows; CrossPlay(behaviour=True) -- nothing played changes, eager
== graph, the counts equal host bookkeeping from the oracle; shards add up; bad arguments.  Every comparison is integer
equality."""
import collections
import ctypes as C

import numpy as np
import pytest
import torch

import behaviour_cases as bc

pytestmark = pytest.mark.gpu
SENTINEL = -0x0123456789abcdef
TAIL = 64


@pytest.fixture(scope="module")
def fa():
    import emergent_multiagent_strategies_amd as m
    assert torch.cuda.is_available()
    m._lib.load()
    return m


def _cells(E, seed):
    """Cells 0, 2, 3 of four (cell 1 has no env); from eight envs on, three envs of cell -1 and one of cell 4 (counted nowhere)."""
    rng = np.random.RandomState(seed)
    cell = rng.choice([0, 2, 3], size=E).astype(np.int32)
    if E >= 8:
        out = rng.choice(E, 4, replace=False)
        cell[out[:3]], cell[out[3]] = -1, 4
    return cell


def _run_case(fa, G, A, E, T, MT, quota, seed, time_step=None, n_chunks=2):
    """A handle from close_state, `n_chunks` open-loop rollouts of T random-action steps with after_update between them, the
    behaviour pass after each; every chunk compared with the restatement on the storage's own rows.  -> (counts, history)."""
    beh = fa.behaviour
    N, n_cells = G + A, 4
    eng = fa.BatchedFortAttack(E, G, A, MT, base_seed=seed)
    st = fa.JointRolloutStorage(T, E, N, device="cuda")
    eng.bind_storage(st)
    eng.collect_reset()
    state = bc.close_state(E, G, A, seed)
    if time_step is not None:
        state["time_step"] = np.asarray(time_step, np.int32)
    eng.set_state(state)
    st.obs[0] = torch.from_numpy(bc.state_obs(state)).cuda()
    cell = _cells(E, seed)
    words = eng.behaviour_cell_words()
    assert words == beh.cell_words(MT)
    buf = torch.full((n_cells * words + TAIL,), SENTINEL, dtype=torch.int64, device="cuda")
    bm = beh.BehaviourMaps(eng, cell, n_cells, quota, counts=buf)
    bm.begin()
    host = buf.cpu().numpy()
    assert not host[:n_cells * words].any() and (host[n_cells * words:] == SENTINEL).all()     # begin zeroes exactly the record
    ep_count, ep_t = bm.episode_counters()
    assert not ep_count.any() and np.array_equal(ep_t, state["time_step"])
    want = beh.new_counts(n_cells, MT)
    ep_count, ep_t = ep_count.astype(np.int64), ep_t.astype(np.int64)
    history = []
    for k in range(n_chunks):
        if k:
            eng.after_update()
        acts = bc.random_actions(np.random.RandomState(1000 * seed + k), (T, E, N))
        st.actions.copy_(torch.from_numpy(acts).cuda().unsqueeze(-1))
        eng.collect_rollout(0, T, auto_reset=True)
        bm.chunk()
        torch.cuda.synchronize()
        obs, done = st.obs.cpu().numpy(), st.done.cpu().numpy()
        before = ep_count.copy()
        beh.behaviour_chunk_numpy(obs, acts, done, cell, ep_count, ep_t, want, G, MT, quota=quota, world=eng.cfg.world)
        history.append((before, ep_count.copy(), done))
        host = buf.cpu().numpy()
        assert (host[n_cells * words:] == SENTINEL).all(), "the pass wrote behind the record"
        bc.assert_counts_equal(bm.counts(), want)                   # every word of the record
        got_count, got_t = bm.episode_counters()
        assert np.array_equal(got_count, ep_count) and np.array_equal(got_t, ep_t), k
    assert np.array_equal(bm.raw().cpu().numpy(), host[:n_cells * words].reshape(n_cells, words))
    eng.close()
    return want, history


@pytest.mark.parametrize("E", [1, 33, 70])
@pytest.mark.parametrize("G,A", [(3, 3), (5, 5), (1, 3), (8, 8), (2, 4)])
def test_kernel_equals_the_restatement(fa, G, A, E):
    """T = 1 (one row), 9 (a partial block) and 129 (three blocks of the scan, the last of one row), without a quota and with
    2 episodes per env; E = 1, 33 (three slices of three cells, partial ones) and 70 (a cell of more than one full slice).  The
    non-triviality conditions need rows to happen in: they are asserted where T = 129 and E >= 33 -- at T = 1 nothing can die
    and be seen dead, with one env nothing is certain."""
    MT = 12
    for T in (1, 9, 129):
        for quota in (0, 2):
            counts, history = _run_case(fa, G, A, E, T, MT, quota, seed=7 + G + 3 * A + E)
            if T == 129 and E >= 33:
                bc.assert_not_trivial(counts, MT, quota, history)
            assert not any(counts[k][1].any() for k in counts)     # the cell without an env
            if quota == 0:
                tabled = int(((_cells(E, 7 + G + 3 * A + E) >= 0) & (_cells(E, 7 + G + 3 * A + E) < 4)).sum())
                assert counts["steps"].sum() == 2 * T * tabled


def test_kernel_with_the_largest_record(fa):
    """max_time_steps = 1024: 43 016 bytes of LDS for the record; envs that start deep into an episode reach the last entries of
    alive_t / len_hist (an episode that starts at step 1000 ends at its timeout inside the second chunk)."""
    E, T, MT = 8, 40, 1024
    time_step = np.array([0, 1000, 1023, 990, 5, 1000, 970, 0], np.int32)
    counts, history = _run_case(fa, 3, 3, E, T, MT, 0, seed=4, time_step=time_step)
    assert counts["alive_t"][:, :, 1000:].sum() > 0 and counts["len_hist"][:, 1023].sum() > 0
    assert counts["occ"].sum() > 0 and counts["shots"].sum() > 0 and counts["deaths"].sum() > 0


def test_hand_made_rows_on_the_device(fa):
    beh = fa.behaviour
    obs, acts, done, cell, ep_t0, want, want_count, want_t = bc.edge_case()
    E = len(cell)
    eng = fa.BatchedFortAttack(E, bc.EDGE_G, bc.EDGE_A, bc.EDGE_MT)
    st = fa.JointRolloutStorage(1, E, 2, device="cuda")
    eng.bind_storage(st)
    eng.collect_reset()
    eng.set_state(dict(time_step=ep_t0))
    st.obs.copy_(torch.from_numpy(obs).cuda())
    st.actions.copy_(torch.from_numpy(acts).cuda().unsqueeze(-1))
    st.done.copy_(torch.from_numpy(done).cuda())
    bm = beh.BehaviourMaps(eng, cell, bc.EDGE_CELLS, 0)
    bm.begin()
    bm.chunk()
    bc.assert_counts_equal(bm.counts(), bc.counter_to_counts(collections.Counter(want), bc.EDGE_CELLS, bc.EDGE_MT))
    got_count, got_t = bm.episode_counters()
    assert np.array_equal(got_count, want_count) and np.array_equal(got_t, want_t)
    # a second begin clears the record and takes ep_t from the world again
    bm.begin()
    assert not bm.raw().any().item() and np.array_equal(bm.episode_counters()[1], ep_t0)


# ---- CrossPlay(behaviour=True) ------------------------------------------------------------------------------------
E3, G3, A3, MAXT3, QUOTA3, SEED3 = 12, 3, 3, 8, 2, 13
_RUNS = {}


def _policy(fa, n, m, seed):
    torch.manual_seed(seed)
    pol = fa.MPNN(num_agents=n, num_opp_agents=m, num_actions=8).cuda().eval()
    for p in pol.parameters():          # non-zero biases, larger logits than the 0.01-gain init gives
        if p.dim() == 1:
            p.data.uniform_(-0.3, 0.3)
        p.requires_grad_(False)
    pol.dist.linear.weight.data.mul_(3.0)
    return pol


def _pools(fa):
    if "pools" not in _RUNS:
        _RUNS["pools"] = ([_policy(fa, G3, A3, 300 + k) for k in range(2)], [_policy(fa, A3, G3, 400 + k) for k in range(2)])
    return _RUNS["pools"]


def _crossplay(fa, E, env_offset, use_graph, behaviour):
    guards, attackers = _pools(fa)
    eng = fa.BatchedFortAttack(E, G3, A3, MAXT3, base_seed=SEED3, env_offset=env_offset)
    return fa.CrossPlay(eng, guards, attackers, QUOTA3, sample_seed=9, use_graph=use_graph, behaviour=behaviour)


def _played(fa, use_graph, behaviour):
    """One evaluation driven chunk by chunk -> dict(raw, chunks: per chunk the storage's obs / actions / done / log-probs /
    values, counts)."""
    key = (use_graph, behaviour)
    if key not in _RUNS:
        cp = _crossplay(fa, E3, 0, use_graph, behaviour)
        cp.begin()
        chunks, remaining = [], E3
        while remaining:
            assert cp.steps_run < QUOTA3 * MAXT3
            if cp.steps_run:
                cp.eng.after_update()
            remaining = cp.run_chunk()
            st = cp.storage
            chunks.append({k: getattr(st, k).cpu().numpy().copy() for k in ("obs", "actions", "done", "action_log_probs", "value_preds")})
        _RUNS[key] = dict(raw=cp.raw().cpu().numpy().copy(), chunks=chunks, counts=cp.behaviour_counts() if behaviour else None,
                          prints=cp.fingerprints() if behaviour else None, cell=cp.cell.cpu().numpy())
    return _RUNS[key]


def test_crossplay_plays_the_same_with_the_option(fa):
    off, on = _played(fa, False, False), _played(fa, False, True)
    assert np.array_equal(off["raw"].view(np.int64), on["raw"].view(np.int64))
    assert len(off["chunks"]) == len(on["chunks"])
    for a, b in zip(off["chunks"], on["chunks"]):
        for k in ("actions", "action_log_probs", "value_preds", "obs", "done"):
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    with pytest.raises(ValueError, match="behaviour=True"):
        _crossplay(fa, E3, 0, False, False).behaviour_counts()


@pytest.mark.parametrize("use_graph", [False, True])
def test_crossplay_behaviour_counts(fa, use_graph):
    from fa_oracle import OracleEnv
    run = _played(fa, use_graph, True)
    counts, raw, n_cells = run["counts"], run["raw"], 4
    assert np.array_equal(counts["episodes"], raw[:, 1].astype(np.int64)) and (counts["episodes"] == QUOTA3 * E3 // n_cells).all()
    assert np.array_equal(counts["len_hist"].sum(1), counts["episodes"])
    assert np.array_equal(counts["alive_t"][:, 0, 0], G3 * counts["episodes"])
    assert np.array_equal(counts["alive_t"][:, 1, 0], A3 * counts["episodes"])
    eager = _played(fa, False, True)
    bc.assert_counts_equal(counts, eager["counts"])                 # eager and graph runs: identical records
    assert np.array_equal(raw.view(np.int64), eager["raw"].view(np.int64))
    # host bookkeeping: the oracle driven by the stored actions, its own observation and done rows
    orc = OracleEnv(E3, G3, A3, MAXT3, base_seed=SEED3)
    row = orc.reset().astype(np.float32)
    cnt, ep_count, ep_t = collections.Counter(), [0] * E3, [0] * E3
    for ch in run["chunks"]:
        T = ch["done"].shape[0]
        obs, done = np.zeros((T + 1, E3, G3 + A3, 6), np.float32), np.zeros((T, E3), np.uint8)
        obs[0] = row
        for s in range(T):
            ref = orc.step(ch["actions"][s, :, :, 0], auto_reset=False)
            d = ref["done"].astype(bool)
            nxt = ref["obs"].copy()
            if d.any():
                nxt[d] = orc.reset(mask=d)[d]
            obs[s + 1], done[s] = nxt.astype(np.float32), ref["done"]
        assert np.array_equal(obs, ch["obs"]) and np.array_equal(done, ch["done"])
        cnt += bc.loop_reference(obs, ch["actions"], done, run["cell"], ep_count, ep_t, n_cells, G3, MAXT3, QUOTA3)
        row = obs[T]
    bc.assert_counts_equal(counts, bc.counter_to_counts(cnt, n_cells, MAXT3))
    assert ep_count == [QUOTA3] * E3
    prints = run["prints"]
    assert prints.shape == (2, 2, len(fa.behaviour.FINGERPRINT_COLUMNS)) and np.isfinite(prints).all()
    assert np.array_equal(prints.reshape(4, -1), fa.behaviour.fingerprint_rows(counts, None))


def test_shards_add_up(fa):
    whole = _crossplay(fa, 60, 0, False, True).run().behaviour_counts()
    parts = [_crossplay(fa, 30, off, False, True).run().behaviour_counts() for off in (0, 30)]
    bc.assert_counts_equal(fa.behaviour.merge_counts(*parts), whole)
    assert (whole["episodes"] == QUOTA3 * 15).all() and whole["occ"].sum() > 0


def test_eval_cli_writes_the_three_kinds_of_files(fa, tmp_path, monkeypatch):
    import sys
    import eval_fortattack_amd as cli
    guards, attackers = _pools(fa)
    for k in range(2):
        torch.save({"models": [guards[k].state_dict(), attackers[k].state_dict()]}, str(tmp_path / ("ep%d.pt" % (k + 1))))
    out = tmp_path / "out"
    monkeypatch.setattr(sys, "argv", ["eval_fortattack_amd.py", "--num-guards", "3", "--num-attackers", "3", "--num-processes", "8",
                                      "--num-env-steps", "8", "--num-eval-episodes", "2", "--guard-load-dir", str(tmp_path),
                                      "--guard-ckpts", "1", "2", "--attacker-load-dir", str(tmp_path), "-l", "1", "2",
                                      "--out-dir", str(out), "--behaviour"])
    cli.main()
    z = np.load(str(out / "behaviour.npz"))
    cols = list(fa.behaviour.FINGERPRINT_COLUMNS)
    assert z["columns"].tolist() == cols and z["fingerprints"].shape == (2, 2, len(cols))
    assert z["occ"].shape == (2, 2, 2, 32, 40) and z["len_hist"].shape == (2, 2, 8) and z["steps"].shape == (2, 2)
    assert (z["episodes"] == 2 * 2).all() and z["occ"].sum() > 0            # two envs per match-up, two episodes each
    lines = open(str(out / "fingerprints.csv")).read().splitlines()
    assert lines[0].split(",") == ["guard", "attacker"] + cols and [ln.split(",")[:2] for ln in lines[1:]] == [
        ["1", "1"], ["1", "2"], ["2", "1"], ["2", "2"]]
    assert np.allclose(np.array([ln.split(",")[2:] for ln in lines[1:]], float), z["fingerprints"].reshape(4, -1), rtol=1e-5)
    for g in (1, 2):
        for a in (1, 2):
            assert (out / ("behaviour_g%d_a%d.png" % (g, a))).stat().st_size > 0
    assert (out / "crossplay.npz").exists()


def test_bad_arguments_are_reported(fa):
    lib = fa._lib.load()
    E = 8
    eng = fa.BatchedFortAttack(E, 2, 3, 10, track_counters=False)   # (the record does not need the counters)
    cell = torch.zeros(E, dtype=torch.int32, device="cuda")
    buf = torch.zeros(4096 * eng.behaviour_cell_words(), dtype=torch.int64, device="cuda")
    cp, bp = C.c_void_p(cell.data_ptr()), C.c_void_p(buf.data_ptr())
    assert lib.fa_behaviour_chunk(eng._h, None) == -3 and b"no storage bound" in lib.fa_last_error()
    eng.bind_storage(fa.JointRolloutStorage(4, E, 5, device="cuda"))
    assert lib.fa_behaviour_chunk(eng._h, None) == -3 and b"fa_behaviour_begin" in lib.fa_last_error()
    assert lib.fa_behaviour_state(eng._h, None, None) == -3 and b"fa_behaviour_begin" in lib.fa_last_error()
    for args, word in (((None, 1, 0, bp), b"null"), ((cp, 1, 0, None), b"null"), ((cp, 0, 0, bp), b"n_cells"),
                       ((cp, 4097, 0, bp), b"n_cells"), ((cp, 1, -1, bp), b"episodes_per_env")):
        assert lib.fa_behaviour_begin(eng._h, args[0], args[1], args[2], args[3], None) == -1, args
        assert word in lib.fa_last_error() and b"fa_behaviour_begin" in lib.fa_last_error()
    assert lib.fa_behaviour_chunk(eng._h, None) == -3                # a refused begin begins nothing
    assert lib.fa_behaviour_begin(eng._h, cp, 4096, 0, bp, None) == 0 and lib.fa_behaviour_chunk(eng._h, None) == 0
    torch.cuda.synchronize()
    with pytest.raises(fa.FaError, match="fa_behaviour_begin"):
        fa.BehaviourMaps(eng, cell, 0).begin()
    long_eng = fa.BatchedFortAttack(E, 2, 3, 1025)
    assert lib.fa_behaviour_begin(long_eng._h, cp, 1, 0, bp, None) == -1 and b"max_time_steps" in lib.fa_last_error()
