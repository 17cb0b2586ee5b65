"""CPU: the host side of episode recording -- split_episodes on hand-made done patterns, the npz / gif writers, the
recorder's 2 GiB refusal, the evaluation script's --record flags and fa_render_io's layout against the header."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def record():
    from emergent_multiagent_strategies_amd import record as r
    return r


def _frames(S, K=1, size=2):
    """Frame t of env k is filled with the value 10 * k + t: a frame names itself."""
    f = np.zeros((S + 1, K, size, size, 3), np.uint8)
    for t in range(S + 1):
        for k in range(K):
            f[t, k] = 10 * k + t
    return f


def _ids(episodes):
    return [[int(f[0, 0, 0]) for f in ep] for ep in episodes]


def test_split_done_at_the_last_step_of_a_chunk(record):
    done = np.zeros((4, 1), np.uint8)
    done[3, 0] = 1                                    # steps 0..3 are one episode; frame 4 would start the next one
    (eps,) = record.split_episodes(_frames(4), done, 3)
    assert _ids(eps) == [[0, 1, 2, 3]]
    assert eps[0].shape == (4, 2, 2, 3) and eps[0].dtype == np.uint8


def test_split_two_dones_in_a_row(record):
    done = np.array([0, 1, 1, 0, 1], np.uint8)[:, None]
    (eps,) = record.split_episodes(_frames(5), done, 5)
    assert _ids(eps) == [[0, 1], [2], [3, 4]]         # a one-step episode is its reset frame alone


def test_split_quota_reached_mid_chunk_drops_the_rest(record):
    done = np.array([0, 1, 0, 1, 0, 1], np.uint8)[:, None]
    (eps,) = record.split_episodes(_frames(6), done, 2)
    assert _ids(eps) == [[0, 1], [2, 3]]
    assert record.split_episodes(_frames(6), done, 0) == [[]]


def test_split_drops_a_trailing_partial_episode_and_treats_envs_independently(record):
    done = np.zeros((5, 2), np.uint8)
    done[1, 0] = 1                                    # env 0: one episode, then three steps of an unfinished one
    got = record.split_episodes(_frames(5, K=2), done, 3)   # env 1 never finishes
    assert _ids(got[0]) == [[0, 1]] and got[1] == []
    with pytest.raises(ValueError, match="split_episodes"):
        record.split_episodes(_frames(5, K=2), done[:4], 3)


def test_write_npz_round_trip(record, tmp_path):
    rng = np.random.default_rng(0)
    eps = [rng.integers(0, 256, (L, 8, 8, 3), dtype=np.uint8) for L in (3, 1)]
    path = str(tmp_path / "v.npz")
    record.write_npz(path, eps)
    with np.load(path) as z:
        assert sorted(z.files) == ["ep0", "ep1"]
        assert all(np.array_equal(z["ep%d" % i], ep) and z["ep%d" % i].dtype == np.uint8 for i, ep in enumerate(eps))


def test_write_gif_round_trip(record, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    frames = np.zeros((5, 24, 24, 3), np.uint8)
    for t in range(5):
        frames[t, 4 * t:4 * t + 4, :, 1] = 255       # a green bar that moves: no two frames alike
    path = str(tmp_path / "v.gif")
    record.write_gif(path, frames, fps=10)
    with Image.open(path) as im:
        assert im.format == "GIF" and im.size == (24, 24) and im.n_frames == 5
        im.seek(3)
        rgb = np.asarray(im.convert("RGB"))
        assert rgb[12:16].min(axis=(0, 1)).tolist() == [0, 255, 0] and rgb[:12].max() == 0
    with pytest.raises(ValueError, match="write_gif"):
        record.write_gif(path, frames[0])


def test_recorder_refuses_more_than_two_gib_before_it_touches_the_device(record):
    eng = types.SimpleNamespace(E=4096, device="cpu")
    with pytest.raises(ValueError, match=r"4\.42 GiB.*limit 2 GiB"):      # 101 x 128 x 350 x 350 x 3 bytes
        record.EpisodeRecorder(eng, np.arange(128), 100, size=350)
    with pytest.raises(ValueError, match="env_index"):
        record.EpisodeRecorder(eng, [4096], 10)


def test_eval_script_record_flags():
    import eval_fortattack_amd as ev
    a = ev.get_args([])
    assert a.record is False
    a = ev.get_args(["--record"])
    assert (a.record, a.video_format, a.record_size, a.record_per_cell, a.record_episodes) == (True, "gif", 128, 1, 1)
    a = ev.get_args(["--record", "--video-format", "npz", "--record-size", "64", "--record-per-cell", "2", "--record-episodes", "3"])
    assert (a.video_format, a.record_size, a.record_per_cell, a.record_episodes) == ("npz", 64, 2, 3)
    with pytest.raises(SystemExit):
        ev.get_args(["--record", "--record-episodes", "4"])             # more than --num-eval-episodes (3)
    with pytest.raises(SystemExit):
        ev.get_args(["--record", "--video-format", "mp4"])


def test_render_io_layout_matches_header(tmp_path):
    """sizeof / offsetof of fa_render_io from a C translation unit including the header == the ctypes struct."""
    from emergent_multiagent_strategies_amd import _lib
    fields = [n for n, _ in _lib.RenderIO._fields_]
    prog = ["#include <stdio.h>", "#include <stddef.h>", '#include "fortattack.h"', "int main(void){",
            'printf("sizeof %zu\\n", sizeof(fa_render_io));']
    prog += ['printf("%s %%zu\\n", offsetof(fa_render_io, %s));' % (f, f) for f in fields]
    prog.append("return 0;}")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(prog))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.RenderIO)
    assert len(fields) == 12
    for f in fields:
        assert int(got[f]) == getattr(_lib.RenderIO, f).offset, f
