"""The bytes of the collector tail, pinned: SHA-256 of every output tensor of every collector-tail entry point
(fa_gae, fa_gae_moments, fa_gae_normalize, fa_adv_moments_onepass, fa_adv_stats, fa_adv_mean_std, fa_adv_moments,
fa_adv_normalize, fa_adv_merge, fa_adv_merge_normalize) against tests/golden/collector_tail_bits.json.

The other collector tests compare the moments to 1e-12 or compare the routes with each other; none of them notices all
routes moving together.  The kernels are documented as bitwise reproducible, so the digests are also compared between two
runs in one process.

The shapes are the smallest that reach every kernel of csrc/fa_collect.hip (dispatch: fa_launch_gae, fa_gae_mom_blocks,
fa_launch_adv_onepass).  The fixture is written by `python tests/test_gpu_collector_bits.py --record` on the GPU; it is
recorded once per intended change of the arithmetic, never to make a refactor pass.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "collector_tail_bits.json")
GAMMA, TAU = 0.99, 0.95
RANKS = 3   # the gathered input of the merges: three refills of the storage

SHAPES = [  # E, G, A, T                  columns
    (37, 2, 5, 33),     # 259      fused scan, ragged N = 7, two chunks; non-vector two-pass
    (11, 3, 3, 65),     # 66       fused scan, second workgroup with two lanes, three chunks (the last of one step)
    (8, 5, 5, 4),       # 80       fused scan; <..., 10> two-pass
    (5462, 3, 3, 4),    # 32 772   first shape past the fused scan: fa_gae_coop_kernel + fa_adv_onepass_vec_kernel<6> (even rows)
    (5463, 3, 3, 3),    # 32 778   the same with odd rows: fa_adv_onepass_kernel
    (3277, 5, 5, 2),    # 32 770   fa_adv_onepass_vec_kernel<10>
    (21846, 3, 3, 2),   # 131 076  fa_gae_kernel
    (43692, 3, 3, 2),   # 262 152  fa_gae4_kernel
]


def _key(shape):
    return "%dx%dx%dx%d" % shape


def _seed(shape):
    E, G, A, T = shape
    return 1000 * T + E % 1000 + G


def _fill(rng, E, N, T):
    """One filling of the storage: finite values, done with p = 0.3, masks with p = 0.8, old returns present."""
    return dict(rewards=rng.randn(T, E, N, 1).astype(np.float32),
                value_preds=rng.randn(T + 1, E, N, 1).astype(np.float32),
                masks=(rng.rand(T + 1, E, N, 1) < 0.8).astype(np.float32),
                returns=rng.randn(T + 1, E, N, 1).astype(np.float32),
                done=(rng.rand(T, E) < 0.3).astype(np.uint8))


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def digests(fa, shape):
    """{'<call>/<output>': sha256} for one shape."""
    import torch
    E, G, A, T = shape
    N = G + A
    rng = np.random.RandomState(_seed(shape))
    eng = fa.BatchedFortAttack(E, G, A, 50)
    st = fa.JointRolloutStorage(T, E, N, device="cuda")
    eng.bind_storage(st)
    out = {}

    def load(data):
        for k, v in data.items():
            getattr(st, k).copy_(torch.from_numpy(v).cuda())

    def put(call, **tensors):
        for name, t in tensors.items():
            out[call + "/" + name] = _sha(t)

    data = _fill(rng, E, N, T)
    load(data)
    eng.gae(GAMMA, TAU)
    put("gae", returns=st.returns)
    # the statistics of the storage as fa_gae left it
    mom, mean, std = eng.adv_moments_onepass()
    put("adv_moments_onepass", moments=mom, mean=mean, std=std)
    s0 = eng.adv_stats(0)
    put("adv_stats0", stats=s0)
    mean0 = (s0[:, 1] / s0[:, 0]).contiguous()
    s1 = eng.adv_stats(1, mean=mean0, out=s0.clone())
    put("adv_stats1", stats=s1)
    mean, std = [x.clone() for x in eng.adv_mean_std()]
    put("adv_mean_std", mean=mean, std=std)
    put("adv_moments", moments=eng.adv_moments())
    put("adv_normalize", adv=eng.adv_normalize(mean, std))
    load(data)
    mom, mean, std = eng.gae_moments(GAMMA, TAU)
    put("gae_moments", returns=st.returns, moments=mom, mean=mean, std=std)
    load(data)
    adv, mom, mean, std = eng.gae_normalize(GAMMA, TAU, out=torch.full((T, E, N, 1), float("nan"), device="cuda"))
    put("gae_normalize", returns=st.returns, adv=adv, moments=mom, mean=mean, std=std)
    # the merges: three refills as three ranks; the storage keeps the last one
    gathered = torch.zeros((RANKS, N, 3), dtype=torch.float64, device="cuda")
    for r in range(RANKS):
        load(_fill(rng, E, N, T))
        eng.gae(GAMMA, TAU)
        eng.adv_moments(out=gathered[r])
    mean, std = eng.adv_merge(gathered)
    put("adv_merge", mean=mean, std=std)
    adv, mean, std = eng.adv_merge_normalize(gathered, out=torch.full((T, E, N, 1), float("nan"), device="cuda"))
    put("adv_merge_normalize", adv=adv, mean=mean, std=std)
    return out


@pytest.fixture(scope="module")
def fa():
    import torch
    import emergent_multiagent_strategies_amd as m
    assert torch.cuda.is_available()
    m._lib.load()
    return m


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)["digests"]


@pytest.mark.parametrize("shape", SHAPES, ids=_key)
def test_collector_tail_bits(fa, recorded, shape):
    got = digests(fa, shape)
    want = recorded[_key(shape)]
    assert sorted(got) == sorted(want)
    moved = [k for k in sorted(got) if got[k] != want[k]]
    assert not moved, "outputs whose bytes differ from the fixture: %s" % moved
    again = digests(fa, shape)
    assert again == got, "not reproducible run to run: %s" % [k for k in sorted(got) if got[k] != again[k]]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: test_gpu_collector_bits.py --record   (on the GPU; rewrites %s)" % os.path.relpath(FIXTURE))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import emergent_multiagent_strategies_amd as m
    m._lib.load()
    rec = {"gamma": GAMMA, "tau": TAU, "ranks": RANKS, "digests": {_key(s): digests(m, s) for s in SHAPES}}
    with open(FIXTURE, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d digests for %d shapes" % (sum(len(v) for v in rec["digests"].values()), len(SHAPES)))
