#!/usr/bin/env python
"""tests/golden/attn_h128.npz: the reference MPNN's attention maps (policy.attn_mat / policy.opp_attn_mat, mpnn.py:139-140,
:158-166 -- what Learner.act returns as attn_list and env.render draws) for the inputs of two fixtures that already exist.

Needs the reference tree (oracle/ref_harness.py imports it unmodified; build container only).  Every case runs the reference
`MPNN._fwd` twice on the same input -- in float32, as shipped, and with the module and the input cast to float64 -- and stores

    <case>.team   float64 (B, n, n)   the LAST message-passing round's softmax weights (`messages(..., return_attn=True)`)
    <case>.opp    float64 (B, n, m)   the opponent attention's (`oppAttn(..., return_attn=True)`)
    <case>.eps    float64 (2,)        max |float32 - float64| of the two: the reference's own rounding noise on this input,
                                      the unit the tests' bounds are written in

Cases: ep<E> = the five published attacker policies on the observations of attackers_tmp1.npz (5v5, B = 64, attackers'
side; weights read from that fixture, where they are data); 3v3.g / 3v3.a / 5v5.g / 5v5.a = both teams of the two cases
of mpnn_h128.npz, weights re-made from the seeds as oracle/gen_golden.py gen_mpnn_h128_fixture makes them (fingerprints
checked against the fixture's).  b1.* records what the reference leaves in attn_mat / opp_attn_mat for a batch of ONE env
(3v3 guards, first observation row): its squeeze(0).squeeze(0) drops the batch axis there, and only there.

    python tools/gen_attn_golden.py            # rewrites tests/golden/attn_h128.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
GOLDEN = os.path.join(ROOT, "tests", "golden")


class _Sp(object):
    shape = (8,)


def _ref_attention(net, obs, own, opp, torch):
    """The reference's _fwd on obs[:, own] / obs[:, opp] (agent-major, as learner.py:150-152 cats them), float32 and float64
    -> (team64, opp64, eps (2,), the float32 pair as the reference left it)."""
    got = []
    for dt in (torch.float32, torch.float64):
        net.to(dt)
        inp = obs[:, own].transpose(0, 1).reshape(-1, 6).to(dt)
        oin = obs[:, opp].transpose(0, 1).reshape(-1, 6).to(dt)
        with torch.no_grad():
            net._fwd(inp, oin, None)
        got.append((np.array(net.attn_mat), np.array(net.opp_attn_mat)))
    net.to(torch.float32)
    (t32, o32), (t64, o64) = got
    assert t32.dtype == np.float32 and t64.dtype == np.float64 and o64.dtype == np.float64
    eps = np.array([np.abs(t32.astype(np.float64) - t64).max(), np.abs(o32.astype(np.float64) - o64).max()])
    return t64, o64, eps, (t32, o32)


def generate():
    """-> dict of arrays (nothing is written)."""
    import torch
    import ref_harness as rh
    import gen_golden as gg
    rh.import_reference()
    torch.set_num_threads(1)
    from mpnn import MPNN

    def new(n, m):
        return MPNN(action_space=_Sp(), num_agents=n, num_opp_agents=m, num_entities=0, input_size=6, pos_index=2,
                    mask_dist=None, entity_mp=False, policy_layers=1)

    rec = {}
    # ---- the published attackers (weights are data in attackers_tmp1.npz)
    z = np.load(os.path.join(GOLDEN, "attackers_tmp1.npz"))
    G, A, B = [int(v) for v in z["meta"]]
    obs = torch.from_numpy(z["obs"])
    for e in [int(e) for e in z["episodes"]]:
        net = new(A, G)
        pre = "ep%d." % e
        net.load_state_dict({k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre) and ".out." not in k})
        t, o, eps, _ = _ref_attention(net, obs, slice(G, G + A), slice(0, G), torch)
        assert t.shape == (B, A, A) and o.shape == (B, A, G)
        rec["ep%d.team" % e], rec["ep%d.opp" % e], rec["ep%d.eps" % e] = t, o, eps
    # ---- both teams of the seed-constructed full-size policies of mpnn_h128.npz
    h = np.load(os.path.join(GOLDEN, "mpnn_h128.npz"))
    for tag in ("3v3", "5v5"):
        G, A, seed, B = [int(v) for v in h[tag + ".meta"]]
        N = G + A
        torch.manual_seed(seed)
        nets = []
        for (n, m), key in (((G, A), ".fingerprint_g"), ((A, G), ".fingerprint_a")):
            net = new(n, m)
            gg.mpnn_h128_setup(net, torch)
            fp, ref = gg.mpnn_fingerprint(net, np), h[tag + key]
            assert (np.abs(fp[:, :2] - ref[:, :2]).max(1) <= 1e-6 * ref[:, 1] + 1e-6).all() and \
                np.abs(fp[:, 2:] - ref[:, 2:]).max() < 1e-5, "the seed did not give the fixture's weights"
            nets.append(net)
        obs = torch.from_numpy(h[tag + ".obs"])
        for net, side, own, opp in ((nets[0], "g", slice(0, G), slice(G, N)), (nets[1], "a", slice(G, N), slice(0, G))):
            t, o, eps, _ = _ref_attention(net, obs, own, opp, torch)
            n = own.stop - own.start
            assert t.shape == (B, n, n) and o.shape == (B, n, N - n)
            c = "%s.%s" % (tag, side)
            rec[c + ".team"], rec[c + ".opp"], rec[c + ".eps"] = t, o, eps
        if tag == "3v3":   # one env: the shapes as the reference leaves them
            t, o, eps, (t32, o32) = _ref_attention(nets[0], obs[:1], slice(0, G), slice(G, N), torch)
            rec["b1.team"], rec["b1.opp"], rec["b1.eps"] = t, o, eps
            rec["b1.team_shape"] = np.array(t32.shape, np.int64)
            rec["b1.opp_shape"] = np.array(o32.shape, np.int64)
    return rec


if __name__ == "__main__":
    out = generate()
    np.savez_compressed(os.path.join(GOLDEN, "attn_h128.npz"), **out)
    for k in sorted(out):
        if k.endswith(".eps"):
            print("%-8s eps team %.2e opp %.2e   largest weight %.4f" % (k[:-4], out[k][0], out[k][1],
                                                                        max(out[k[:-4] + ".team"].max(), out[k[:-4] + ".opp"].max())))
    print("b1 shapes", out["b1.team_shape"].tolist(), out["b1.opp_shape"].tolist())
