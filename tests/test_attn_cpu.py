"""CPU: the attention maps of the policies (the reference's policy.attn_mat / opp_attn_mat, mpnn.py:139-140, :158-166; what
Learner.act returns as attn_list and env.render draws) -- the C structure that carries them, this repo's PyTorch module
against the reference's float64 matrices (tests/golden/attn_h128.npz, tools/gen_attn_golden.py), and the renderer's overlay
(fortattack.py:439-466, :531-546).

Bound against the fixture: absolute (the weights live in [0, 1]), 8 x eps of the case, eps = the reference's own
max |float32 - float64| on that input, read from the fixture.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATTACKER_CASES = ["ep220", "ep650", "ep1240", "ep1600", "ep2520"]
H128_CASES = ["3v3.g", "3v3.a", "5v5.g", "5v5.a"]


@pytest.fixture(scope="module")
def fa():
    import emergent_multiagent_strategies_amd as m
    return m


@pytest.fixture(scope="module")
def attn_golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "attn_h128.npz"))
    return {k: z[k] for k in z.files}


def test_policy_io_layout_matches_header(fa, tmp_path):
    """sizeof / offsetof of fa_policy_io from a C translation unit including the header == _lib.PolicyIO."""
    fields = ["obs", "weights", "seed", "value_only", "attacker_pool", "pool_size", "env_strategy", "team_attn", "opp_attn"]
    prog = ["#include <stdio.h>", "#include <stddef.h>", '#include "fortattack.h"', "int main(void){",
            'printf("sizeof %zu\\n", sizeof(fa_policy_io));']
    for f in fields:
        prog.append('printf("%s %%zu\\n", offsetof(fa_policy_io, %s));' % (f, f))
    prog.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["sizeof"]) == C.sizeof(fa._lib.PolicyIO)
    for f in fields:
        assert int(got[f]) == getattr(fa._lib.PolicyIO, f).offset, f
    io = fa._lib.PolicyIO()                                  # zero-initialised = no export, as before the fields existed
    assert not any(io.team_attn[t] or io.opp_attn[t] for t in range(2))
    assert fa._lib.PolicyIO.team_attn.size == fa._lib.PolicyIO.opp_attn.size == 2 * C.sizeof(C.c_void_p)


def _check_maps(team, opp, n, m, B):
    """Shapes, an exactly-zero diagonal, rows summing to 1 (a team of one: the 1 x 1 zero)."""
    assert team.shape == (B, n, n) and opp.shape == (B, n, m)
    assert (np.diagonal(team, axis1=1, axis2=2) == 0.0).all()
    if n >= 2:
        assert np.abs(team.astype(np.float64).sum(-1) - 1.0).max() <= 1e-6
    else:
        assert (team == 0.0).all()
    assert np.abs(opp.astype(np.float64).sum(-1) - 1.0).max() <= 1e-6
    assert team.min() >= 0.0 and opp.min() >= 0.0


def _module_maps(pol, own, opp):
    with torch.no_grad():
        _, team, oa = pol.trunk(own, opp, return_attn=True)
    return team.numpy(), oa.numpy()


def _assert_within(got, want, eps, what):
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("%s: max |module - float64 reference| = %.3e, bound 8 x eps = %.3e" % (what, err, 8 * eps))
    assert want.dtype == np.float64 and eps > 0
    assert err <= 8 * eps, what


def test_module_matches_the_reference_for_the_published_attackers(fa, golden_dir, attn_golden):
    from test_mpnn_cpu import attacker_pool_from_golden
    z, pool, G, A = attacker_pool_from_golden(fa.MPNN, golden_dir)
    obs = torch.from_numpy(z["obs"])
    assert ["ep%d" % int(e) for e in z["episodes"]] == ATTACKER_CASES
    for case, pol in zip(ATTACKER_CASES, pool):
        team, opp = _module_maps(pol, obs[:, G:], obs[:, :G])
        _check_maps(team, opp, A, G, obs.shape[0])
        _assert_within(team, attn_golden[case + ".team"], attn_golden[case + ".eps"][0], case + " team")
        _assert_within(opp, attn_golden[case + ".opp"], attn_golden[case + ".eps"][1], case + " opp")
    # sharp softmaxes are in the fixture: a real test of the exponentials, not near-uniform weights
    assert max(attn_golden[c + ".team"].max() for c in ATTACKER_CASES) > 0.99


@pytest.mark.parametrize("tag", ["3v3", "5v5"])
def test_module_matches_the_reference_at_full_size(fa, golden_dir, attn_golden, tag):
    from test_mpnn_cpu import h128_policies
    g = np.load(os.path.join(golden_dir, "mpnn_h128.npz"))
    pols, G, A = h128_policies(fa.MPNN, g, tag)
    obs = torch.from_numpy(g[tag + ".obs"])
    for pol, side, own, opp in ((pols[0], "g", obs[:, :G], obs[:, G:]), (pols[1], "a", obs[:, G:], obs[:, :G])):
        case = "%s.%s" % (tag, side)
        team, oa = _module_maps(pol, own, opp)
        _check_maps(team, oa, own.shape[1], opp.shape[1], obs.shape[0])
        _assert_within(team, attn_golden[case + ".team"], attn_golden[case + ".eps"][0], case + " team")
        _assert_within(oa, attn_golden[case + ".opp"], attn_golden[case + ".eps"][1], case + " opp")


def test_single_env_shapes_are_the_references(fa, golden_dir, attn_golden):
    """B = 1: the reference's squeeze(0).squeeze(0) leaves (n, n) / (n, m); the module keeps its batch axis and the learner's
    numpy format (collapse a batch of one) gives the reference's shape."""
    from test_mpnn_cpu import h128_policies
    g = np.load(os.path.join(golden_dir, "mpnn_h128.npz"))
    pols, G, A = h128_policies(fa.MPNN, g, "3v3")
    obs = torch.from_numpy(g["3v3.obs"])[:1]
    team, opp = _module_maps(pols[0], obs[:, :G], obs[:, G:])
    _check_maps(team, opp, G, A, 1)
    assert tuple(attn_golden["b1.team_shape"]) == team[0].shape == (G, G)
    assert tuple(attn_golden["b1.opp_shape"]) == opp[0].shape == (G, A)
    _assert_within(team[0], attn_golden["b1.team"], attn_golden["b1.eps"][0], "b1 team")
    _assert_within(opp[0], attn_golden["b1.opp"], attn_golden["b1.eps"][1], "b1 opp")


@pytest.mark.parametrize("n,m", [(1, 3), (4, 1)])
def test_team_of_one(fa, n, m):
    """mpnn.py:266-274: a team of one attends to nobody (a zero 1 x 1 matrix); a single opponent gets all the weight."""
    torch.manual_seed(n * 10 + m)
    pol = fa.MPNN(num_agents=n, num_opp_agents=m, num_actions=8)
    team, opp = _module_maps(pol, torch.randn(7, n, 6), torch.randn(7, m, 6))
    _check_maps(team, opp, n, m, 7)
    if m == 1:
        assert (opp == 1.0).all()


# ---- renderer ---------------------------------------------------------------------------------------------------------
SIZE, AGENT = 400, 0.05
PX = np.array([-0.6, 0.0, 0.6, -0.6, 0.0, 0.6])
PY = np.array([0.4, 0.4, 0.4, -0.4, -0.4, -0.4])
ANG = np.full(6, np.pi / 2)            # heads point up: the probes below sit to the right / at the centre


def _pix(x, y):
    """The pixel whose centre is nearest to world (x, y): (row, col)."""
    return int(np.floor((1.0 - y) * SIZE / 2.0)), int(np.floor((x + 1.0) * SIZE / 2.0))


def _attn_list(row_team, row_opp, k, batch_axis=False):
    team, opp = np.zeros((3, 3)), np.zeros((3, 3))
    team[k], opp[k] = row_team, row_opp
    if batch_axis:
        team, opp = team[None], opp[None]
    return [[team, opp], [np.full((3, 3), 0.5), np.full((3, 3), 0.5)]]       # entry 1, the attackers', is not drawn


def _frame(fa, alive=(1,) * 6, **kw):
    from emergent_multiagent_strategies_amd.render import render_frame
    return render_frame(PX, PY, ANG, np.array(alive), 3, size=SIZE, agent_size=AGENT, **kw)


YELLOW_ON_BLACK = (int(0.9 * 255.0 + 0.5),) * 2 + (0,)       # (1, 1, 0) at alpha 0.9 over the black active region


def test_overlay_draws_the_reference_agents_row(fa):
    """Agent k = 0 (the first alive one) attends: guard 1 with 0.8, guard 2 with 0.1, attacker 3 with 0.1, attacker 4 with
    0.8.  At 1.4 agent radii from an agent's centre: the yellow blend under weight 0.8 (disc radius 1.8), background
    under 0.1 (radius 1.1).  Agent 0's centre: half its team colour."""
    plain = _frame(fa)
    for batch_axis in (False, True):
        img = _frame(fa, attn_list=_attn_list([0.0, 0.8, 0.1], [0.1, 0.8, 0.1], 0, batch_axis))
        d = 1.4 * AGENT
        for i, w in ((1, 0.8), (2, 0.1), (3, 0.1), (4, 0.8), (5, 0.1)):
            r, c = _pix(PX[i] + d, PY[i])
            want = YELLOW_ON_BLACK if w == 0.8 else (0, 0, 0)
            assert tuple(img[r, c]) == want, (i, w)
            assert tuple(plain[r, c]) == (0, 0, 0)
            # the agent's own disc lies on top of the yellow one
            assert tuple(img[_pix(PX[i] - 0.5 * AGENT, PY[i])]) == ((0, 255, 0) if i < 3 else (255, 0, 0))
        assert tuple(img[_pix(PX[0], PY[0])]) == (0, 128, 0)                  # 0.5 * green, alpha 1
        assert tuple(plain[_pix(PX[0], PY[0])]) == (0, 255, 0)
        assert tuple(img[_pix(PX[0] + d, PY[0])]) == (0, 0, 0)                # no disc around the reference agent itself
        # nothing else moved: outside the discs of radius 2 agent sizes the frames are equal
        X, Y = np.meshgrid((np.arange(SIZE) + 0.5) / SIZE * 2 - 1, -((np.arange(SIZE) + 0.5) / SIZE * 2 - 1))
        far = np.ones((SIZE, SIZE), bool)
        for i in range(6):
            far &= (X - PX[i]) ** 2 + (Y - PY[i]) ** 2 > (2.0 * AGENT) ** 2
        assert np.array_equal(img[far], plain[far]) and not np.array_equal(img, plain)


def test_no_attention_is_todays_frame(fa):
    plain = _frame(fa, shoot=np.array([0, 1, 0, 0, 0, 1], bool))
    assert np.array_equal(_frame(fa, shoot=np.array([0, 1, 0, 0, 0, 1], bool), attn_list=None), plain)
    off = _frame(fa, shoot=np.array([0, 1, 0, 0, 0, 1], bool), attn_list=_attn_list([0, 0.8, 0.1], [0.1, 0.8, 0.1], 0),
                 viz_attn=False)
    assert np.array_equal(off, plain)
    # the frame of the renderer before the overlay existed, pinned by a few pixels of it
    assert tuple(plain[_pix(PX[0], PY[0])]) == (0, 255, 0) and tuple(plain[_pix(PX[3], PY[3])]) == (255, 0, 0)
    assert tuple(plain[_pix(0.9, 0.0)]) == (0, 0, 0) and tuple(plain[_pix(0.0, 0.9)]) == (128, 128, 128)


def test_reference_agent_is_the_first_alive_one(fa):
    from emergent_multiagent_strategies_amd.render import attn_reference_agent
    assert attn_reference_agent([1, 1, 1, 1, 1, 1], 3) == 0
    assert attn_reference_agent([0, 1, 1, 1, 1, 1], 3) == 1
    assert attn_reference_agent([0, 0, 0, 0, 0, 0], 3) == 2             # nobody alive: num_guards - 1
    assert attn_reference_agent([0, 0, 0, 1, 1, 1], 3) == 2             # fortattack.py:441-444 stops at the last guard
    # a dead first guard: row 1 is drawn, agent 1 gets the dot, the dead agent 0 is not drawn at all
    d = 1.4 * AGENT
    img = _frame(fa, alive=(0, 1, 1, 1, 1, 1), attn_list=_attn_list([0.8, 0.0, 0.8], [0.1, 0.1, 0.8], 1))
    assert tuple(img[_pix(PX[1], PY[1])]) == (0, 128, 0)
    assert tuple(img[_pix(PX[2] + d, PY[2])]) == YELLOW_ON_BLACK and tuple(img[_pix(PX[5] + d, PY[5])]) == YELLOW_ON_BLACK
    assert tuple(img[_pix(PX[3] + d, PY[3])]) == (0, 0, 0)
    assert tuple(img[_pix(PX[0] + d, PY[0])]) == (0, 0, 0) and tuple(img[_pix(PX[0], PY[0])]) == (0, 0, 0)
    # ... and is drawn, fainter (alpha 0.3), with viz_dead
    img = _frame(fa, alive=(0, 1, 1, 1, 1, 1), viz_dead=True, attn_list=_attn_list([0.8, 0.0, 0.8], [0.1, 0.1, 0.8], 1))
    assert tuple(img[_pix(PX[0] + d, PY[0])]) == (int(0.3 * 255.0 + 0.5),) * 2 + (0,)
    # all dead: k = 2; nothing is drawn without viz_dead, the dot and the row-2 discs with it
    none = _frame(fa, alive=(0,) * 6, attn_list=_attn_list([0.8, 0.8, 0.0], [0.8, 0.8, 0.8], 2))
    assert np.array_equal(none, _frame(fa, alive=(0,) * 6))
    img = _frame(fa, alive=(0,) * 6, viz_dead=True, attn_list=_attn_list([0.8, 0.8, 0.0], [0.8, 0.8, 0.8], 2))
    assert tuple(img[_pix(PX[2], PY[2])]) == (0, 128, 0)
    assert tuple(img[_pix(PX[0] + d, PY[0])]) == (int(0.3 * 255.0 + 0.5),) * 2 + (0,)
    assert tuple(img[_pix(PX[2] + d, PY[2])]) == (0, 0, 0)


def test_overlay_rejects_matrices_of_more_than_one_env(fa):
    bad = [[np.zeros((2, 3, 3)), np.zeros((2, 3, 3))]]
    with pytest.raises(ValueError):
        _frame(fa, attn_list=bad)


def test_render_state_passes_the_attention_through(fa):
    from emergent_multiagent_strategies_amd.render import render_state
    st = dict(pos_x=PX[None], pos_y=PY[None], ang=ANG[None], alive=np.ones((1, 6)))
    al = _attn_list([0.0, 0.8, 0.1], [0.1, 0.8, 0.1], 0)
    assert np.array_equal(render_state(st, 0, 3, size=SIZE, agent_size=AGENT, attn_list=al), _frame(fa, attn_list=al))


# ---- the fixture's generator ------------------------------------------------------------------------------------------
def test_generator_reproduces_the_committed_fixture(attn_golden):
    import ref_harness as rh
    if not rh.reference_available():
        pytest.skip("the reference tree is not present")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_attn_golden
    finally:
        sys.path.pop(0)
    threads = torch.get_num_threads()
    try:
        fresh = gen_attn_golden.generate()
    finally:
        torch.set_num_threads(threads)
    assert sorted(fresh) == sorted(attn_golden)
    for k, v in fresh.items():
        assert v.shape == attn_golden[k].shape and np.abs(np.asarray(v, np.float64) - attn_golden[k]).max() <= 1e-12, k
