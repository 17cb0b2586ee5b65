"""CPU: the behaviour record's definition (behaviour.behaviour_chunk_numpy) against an independently structured loop on
episodes played by the C oracle, hand-made edge rows, the carry of the per-env counters between chunks, the fingerprint
closed forms, merging, the PNG, the CLI flag and the record layout of the header."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import behaviour_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fa():
    import emergent_multiagent_strategies_amd as m
    from emergent_multiagent_strategies_amd import build
    build.build()  # hipcc cross-compiles for gfx950 without a GPU
    return m


def oracle_chunks(E, G, A, MT, T, n_chunks, seed):
    """n_chunks storages (obs (T+1, E, N, 6) float32, actions (T, E, N), done (T, E)) as a collector with auto-reset would
    fill them: the oracle from close_state under random actions; obs[0] of a chunk is obs[T] of the one before."""
    from fa_oracle import OracleEnv
    N = G + A
    orc = OracleEnv(E, G, A, MT, base_seed=seed)
    orc.reset()
    st = bc.close_state(E, G, A, seed)
    orc.set_state(st)
    row = bc.state_obs(st)
    rng = np.random.RandomState(seed + 1)
    chunks = []
    for _ in range(n_chunks):
        obs = np.zeros((T + 1, E, N, 6), np.float32)
        obs[0] = row
        acts = bc.random_actions(rng, (T, E, N))
        done = np.zeros((T, E), np.uint8)
        for s in range(T):
            ref = orc.step(acts[s], auto_reset=False)
            d = ref["done"].astype(bool)
            nxt = ref["obs"].copy()
            if d.any():
                nxt[d] = orc.reset(mask=d)[d]
            obs[s + 1], done[s] = nxt.astype(np.float32), ref["done"]
        chunks.append((obs, acts, done))
        row = obs[T]
    return chunks


E1, G1, A1, MT1, T1, CELLS1 = 6, 3, 3, 12, 20, 3
CELL1 = np.array([0, 2, 0, 2, -1, 0], np.int32)        # cell 1 has no env, env 4 is counted nowhere


@pytest.fixture(scope="module")
def chunks1():
    return oracle_chunks(E1, G1, A1, MT1, T1, 2, seed=5)


@pytest.mark.parametrize("quota", [0, 2])
def test_restatement_equals_an_independent_loop(fa, chunks1, quota):
    beh = fa.behaviour
    counts = beh.new_counts(CELLS1, MT1)
    ep_count, ep_t = np.zeros(E1, np.int64), np.zeros(E1, np.int64)
    ref_count, ref_t = [0] * E1, [0] * E1
    cnt, history = None, []
    for obs, acts, done in chunks1:
        before = ep_count.copy()
        beh.behaviour_chunk_numpy(obs, acts, done, CELL1, ep_count, ep_t, counts, G1, MT1, quota=quota)
        history.append((before, ep_count.copy(), done))
        c = bc.loop_reference(obs, acts, done, CELL1, ref_count, ref_t, CELLS1, G1, MT1, quota)
        cnt = c if cnt is None else cnt + c
    bc.assert_counts_equal(counts, bc.counter_to_counts(cnt, CELLS1, MT1))
    assert ep_count.tolist() == ref_count and ep_t.tolist() == ref_t
    bc.assert_not_trivial(counts, MT1, quota, history)
    assert counts["steps"][1] == 0 and all(counts[k][1].sum() == 0 for k in beh.SECTIONS)       # the cell without an env
    assert counts["len_hist"].sum(1).tolist() == counts["episodes"].tolist()
    if quota:
        assert ep_count.max() == quota                              # nothing is counted beyond the quota
        assert counts["episodes"].sum() == quota * int((CELL1 >= 0).sum())
    else:
        assert counts["steps"].sum() == 2 * T1 * int((CELL1 >= 0).sum())
        assert counts["alive_t"].sum() == counts["occ"].sum()


def test_hand_made_rows(fa):
    beh = fa.behaviour
    obs, acts, done, cell, ep_t0, want, want_count, want_t = bc.edge_case()
    counts = beh.new_counts(bc.EDGE_CELLS, bc.EDGE_MT)
    ep_count, ep_t = np.zeros(len(cell), np.int32), ep_t0.copy()
    beh.behaviour_chunk_numpy(obs, acts, done, cell, ep_count, ep_t, counts, bc.EDGE_G, bc.EDGE_MT, quota=0)
    import collections
    bc.assert_counts_equal(counts, bc.counter_to_counts(collections.Counter(want), bc.EDGE_CELLS, bc.EDGE_MT))
    assert np.array_equal(ep_count, want_count) and np.array_equal(ep_t, want_t)
    # ... and the independent loop reads the same rows the same way
    rc, rt = [0] * len(cell), ep_t0.tolist()
    cnt = bc.loop_reference(obs, acts, done, cell, rc, rt, bc.EDGE_CELLS, bc.EDGE_G, bc.EDGE_MT, 0)
    assert {k: v for k, v in cnt.items() if v} == want and rc == want_count.tolist() and rt == want_t.tolist()


@pytest.mark.parametrize("quota", [0, 1])
def test_two_chunks_equal_one_chunk_of_the_concatenated_rows(fa, quota):
    beh = fa.behaviour
    (obs, acts, done), = oracle_chunks(5, 2, 3, 6, 14, 1, seed=3)
    cell = np.array([1, 0, 1, 5, 0], np.int32)
    whole = beh.new_counts(2, 6)
    wc, wt = np.zeros(5, np.int64), np.array([0, 1, 2, 3, 9], np.int64)
    beh.behaviour_chunk_numpy(obs, acts, done, cell, wc, wt, whole, 2, 6, quota=quota)
    parts = beh.new_counts(2, 6)
    pc, pt = np.zeros(5, np.int64), np.array([0, 1, 2, 3, 9], np.int64)
    for lo in (0, 7):
        beh.behaviour_chunk_numpy(obs[lo:lo + 8], acts[lo:lo + 7], done[lo:lo + 7], cell, pc, pt, parts, 2, 6, quota=quota)
    bc.assert_counts_equal(parts, whole)
    assert np.array_equal(pc, wc) and np.array_equal(pt, wt)
    assert whole["episodes"].sum() > 0 and done[:7].any() and done[7:].any()


def test_fingerprint_rows_closed_forms(fa):
    beh = fa.behaviour
    counts = beh.new_counts(3, 10)
    # cell 0: guards in two bins of one row, attackers in two bins of one column; cell 1 stays empty; cell 2: guards only
    counts["steps"][0], counts["episodes"][0] = 40, 4
    counts["len_hist"][0, 3], counts["len_hist"][0, 9] = 3, 1          # lengths 4, 4, 4, 10
    counts["occ"][0, 0, 31, 19], counts["occ"][0, 0, 31, 23] = 30, 10  # centres x = -0.025, 0.175; y = 0.775
    counts["shots"][0, 0, 31, 19] = 8
    counts["deaths"][0, 0, 31, 23] = 2
    counts["occ"][0, 1, 10, 5], counts["occ"][0, 1, 20, 5] = 6, 18      # centres y = -0.275, 0.225; x = -0.725
    counts["shots"][0, 1, 20, 5] = 12
    counts["steps"][2] = 5
    counts["occ"][2, 0, 0, 0] = 5                                      # far from the door
    rows = beh.fingerprint_rows(counts)
    col = beh.FINGERPRINT_COLUMNS.index
    assert rows.shape == (3, len(beh.FINGERPRINT_COLUMNS)) and rows.dtype == np.float64
    assert not rows[1].any()
    r = rows[0]
    assert r[col("mean_episode_length")] == pytest.approx(5.5)
    assert r[col("guard_shots_per_alive_step")] == pytest.approx(0.2) and r[col("attacker_shots_per_alive_step")] == pytest.approx(0.5)
    assert r[col("guard_deaths_per_alive_step")] == pytest.approx(0.05) and r[col("attacker_deaths_per_alive_step")] == 0
    assert r[col("guard_mean_y")] == pytest.approx(0.775) and r[col("attacker_mean_y")] == pytest.approx(0.1)
    # two points 0.2 apart with weights 3/4 and 1/4: std = 0.2 * sqrt(3/16)
    assert r[col("guard_std_x")] == pytest.approx(0.2 * np.sqrt(3.0 / 16)) and r[col("attacker_std_x")] == pytest.approx(0.0, abs=1e-12)
    # door (0, 0.8), radius 2 * 0.15: both guard bins are within it (distances 0.035.., 0.177..)
    assert r[col("guard_share_near_door")] == pytest.approx(1.0) and r[col("attacker_share_upper_half")] == pytest.approx(0.75)
    assert rows[2, col("guard_share_near_door")] == 0 and rows[2, col("mean_episode_length")] == 0
    assert rows[2, col("guard_mean_y")] == pytest.approx(-0.775) and not rows[2, [col("attacker_mean_y"), col("attacker_std_x")]].any()
    # another world: the bin centres follow its walls
    wide = dict(wall_xmin=-2.0, wall_xmax=2.0, wall_ymin=-0.8, wall_ymax=0.8, fort_dim=0.15, door_x=0.0, door_y=0.8)
    assert beh.fingerprint_rows(counts, wide)[0, col("guard_std_x")] == pytest.approx(0.4 * np.sqrt(3.0 / 16))


def test_merge_counts_is_plain_addition(fa, chunks1):
    beh = fa.behaviour
    obs, acts, done = chunks1[0]
    whole = beh.new_counts(CELLS1, MT1)
    beh.behaviour_chunk_numpy(obs, acts, done, CELL1, np.zeros(E1, np.int64), np.zeros(E1, np.int64), whole, G1, MT1)
    halves = []
    for sl in (slice(0, 3), slice(3, 6)):                           # two shards of three envs
        part = beh.new_counts(CELLS1, MT1)
        beh.behaviour_chunk_numpy(obs[:, sl], acts[:, sl], done[:, sl], CELL1[sl], np.zeros(3, np.int64), np.zeros(3, np.int64),
                                  part, G1, MT1)
        halves.append(part)
    merged = beh.merge_counts(*halves)
    bc.assert_counts_equal(merged, whole)
    assert set(merged) == set(beh.SECTIONS)


def test_unpack_counts_follows_the_record_order(fa):
    beh = fa.behaviour
    MT, words = 5, beh.cell_words(5)
    raw = np.arange(2 * words, dtype=np.uint64)
    got = beh.unpack_counts(raw, 2, MT)
    at = 0
    for k in beh.SECTIONS:
        n = got[k][0].size
        assert np.array_equal(got[k].reshape(2, -1), np.stack([np.arange(at, at + n), words + np.arange(at, at + n)])), k
        at += n
    assert at == words and got["occ"].shape == (2, 2, 32, 40) and got["steps"].shape == (2,)


def test_heatmap_png_round_trip(fa, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    beh = fa.behaviour
    counts = beh.new_counts(1, 4)
    counts["occ"][0, 0, 31, 0] = 4          # guards, top-left bin: the picture's first panel, its top-left pixels
    counts["occ"][0, 0, 0, 39] = 2          # ... bottom-right bin of the same panel at half the level
    counts["deaths"][0, 1, 0, 0] = 9        # attackers, deaths: bottom-left bin of the last panel of the second row
    path = tmp_path / "cell.png"
    beh.write_heatmaps(str(path), {k: v[0] for k, v in counts.items()})
    img = np.asarray(Image.open(str(path)).convert("RGB"))
    S, P = beh.HEATMAP_SCALE, beh.HEATMAP_GAP
    assert img.shape == (2 * 32 * S + P, 3 * 40 * S + 2 * P, 3)
    assert np.array_equal(img, beh.heatmap_image(counts))                    # with the leading axis of one cell as well
    assert img[0, 0].tolist() == [0, 255, 0] and img[S - 1, S - 1].tolist() == [0, 255, 0] and img[S, S].tolist() == [0, 0, 0]
    assert img[32 * S - 1, 40 * S - 1].tolist() == [0, 128, 0]
    assert img[32 * S, 0].tolist() == [128, 128, 128] and img[0, 40 * S].tolist() == [128, 128, 128]      # the gaps
    assert img[-1, 2 * (40 * S + P)].tolist() == [255, 0, 0]
    assert img[0, 40 * S + P].tolist() == [0, 0, 0]                          # an empty panel is black


def test_eval_cli_takes_the_behaviour_flag():
    import eval_fortattack_amd as cli
    assert cli.get_args(["--behaviour"]).behaviour is True and cli.get_args([]).behaviour is False
    assert "--behaviour" in open(os.path.join(ROOT, "eval_fortattack_amd.py")).read().split('"""')[1]      # the header comment


def test_record_layout_matches_the_header(fa, tmp_path):
    """FA_BEHAVIOUR_* from a C translation unit including the header == the Python side's section table."""
    beh = fa.behaviour
    names = dict(steps="FA_BEHAVIOUR_OFF_STEPS", episodes="FA_BEHAVIOUR_OFF_EPISODES", len_hist="FA_BEHAVIOUR_OFF_LEN_HIST",
                 alive_t="FA_BEHAVIOUR_OFF_ALIVE_T(mt)", occ="FA_BEHAVIOUR_OFF_OCC(mt)", shots="FA_BEHAVIOUR_OFF_SHOTS(mt)",
                 deaths="FA_BEHAVIOUR_OFF_DEATHS(mt)", words="FA_BEHAVIOUR_CELL_WORDS(mt)")
    prog = ["#include <stdio.h>", '#include "fortattack.h"', "int main(void){", "static const int mts[] = {1, 12, 100, 1024};",
            'printf("bx %d\\nby %d\\n", FA_BEHAVIOUR_BX, FA_BEHAVIOUR_BY);', "for (int k = 0; k < 4; ++k) { long mt = mts[k];"]
    for k, macro in names.items():
        prog.append('printf("%s.%%ld %%ld\\n", mt, (long)(%s));' % (k, macro))
    prog.append("} return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert (int(got["bx"]), int(got["by"])) == (beh.BX, beh.BY) == (40, 32)
    for mt in (1, 12, 100, 1024):
        off = beh.section_offsets(mt)
        assert list(off) == list(beh.SECTIONS)
        for k in beh.SECTIONS:
            assert int(got["%s.%d" % (k, mt)]) == off[k][0], (k, mt)
        assert int(got["words.%d" % mt]) == beh.cell_words(mt) == 2 + 3 * mt + 6 * 32 * 40
    assert beh.cell_words(1024) * 4 == 43016                                   # the largest LDS record


def test_behaviour_calls_refuse_a_null_handle_by_name(fa):
    lib = fa._lib.load()
    assert lib.fa_behaviour_cell_words.restype is C.c_int64
    assert lib.fa_behaviour_cell_words(None) < 0 and b"fa_behaviour_cell_words" in lib.fa_last_error()
    assert lib.fa_behaviour_begin(None, None, 1, 0, None, None) == -1 and b"fa_behaviour_begin" in lib.fa_last_error()
    assert lib.fa_behaviour_chunk(None, None) == -1 and b"fa_behaviour_chunk" in lib.fa_last_error()
    assert lib.fa_behaviour_state(None, None, None) == -1 and b"fa_behaviour_state" in lib.fa_last_error()
