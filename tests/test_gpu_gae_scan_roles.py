"""GPU parity of fa_gae_mom_kernel, the role-split GAE scan with the advantage-moment partials (loaders that leave
delta / c / reset flag in LDS, a scanning wave that carries the recurrence alone, a post wave one chunk behind it):
returns bit for bit against the numpy collector oracle, moments against numpy fp64, at the smallest shapes where the
three-trip pipeline can go wrong -- every T around the chunk length (fill, drain, a last chunk of one step), a single
workgroup of 4 columns, a second workgroup with two valid lanes, a ragged N = 7 -- and every kind of episode-end pattern.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C = 32   # FA_GAEC_CHUNK (csrc/fa_collect.hip): steps per chunk of the cooperative scan
GAMMA, TAU = 0.99, 0.95


@pytest.fixture(scope="module")
def fa():
    import emergent_multiagent_strategies_amd as m
    assert torch.cuda.is_available()
    m._lib.load()
    return m


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _done_patterns(rng, T, E):
    none = np.zeros((T, E), np.uint8)
    row0, last = none.copy(), none.copy()
    row0[0] = 1
    last[T - 1] = 1
    return {"none": none,
            "all": np.ones((T, E), np.uint8),       # every entry t >= 1 is stale: the on-the-spot gather loop runs
            "row0": row0, "last_row": last,
            "p05": (rng.rand(T, E) < 0.05).astype(np.uint8),
            "p50": (rng.rand(T, E) < 0.50).astype(np.uint8)}


def _mask_patterns(rng, T, E, N):
    shape = (T + 1, E, N, 1)
    return {"ones": np.ones(shape, np.float32), "zeros": np.zeros(shape, np.float32),
            "random": (rng.rand(*shape) > 0.3).astype(np.float32)}


@pytest.mark.parametrize("E,G,A", [(2, 1, 1),      # 4 columns: one workgroup, 60 idle lanes
                                   (11, 3, 3),     # 66 columns: a second workgroup with two valid lanes
                                   (37, 2, 5)])    # 259 columns, N = 7: ragged
@pytest.mark.parametrize("T", [1, 2, C - 1, C, C + 1, 2 * C, 2 * C + 1, 3 * C + 1])
def test_gae_scan_roles_vs_oracle(fa, E, G, A, T):
    import collector_oracle as co
    N = G + A
    rng = np.random.RandomState(1000 * T + E)
    eng = fa.BatchedFortAttack(E, G, A, 50)
    st = fa.JointRolloutStorage(T, E, N, device="cuda")
    eng.bind_storage(st)
    rewards = rng.randn(T, E, N, 1).astype(np.float32)
    rewards[rng.rand(T, E, N, 1) < 0.2] = -0.0
    values = rng.randn(T + 1, E, N, 1).astype(np.float32)
    values[rng.rand(T + 1, E, N, 1) < 0.05] = -0.0
    old_returns = (3.0 * rng.randn(T + 1, E, N, 1)).astype(np.float32)   # stale entries of the previous update
    old_returns[T] = np.nan                                               # any read of row T shows up in the moments
    adv_out = torch.empty((T, E, N, 1), device="cuda")
    for dname, done in _done_patterns(rng, T, E).items():
        for mname, masks in _mask_patterns(rng, T, E, N).items():
            tag = "%s/%s" % (dname, mname)
            data = dict(rewards=rewards, value_preds=values, masks=masks, returns=old_returns, done=done)

            def load():
                for k, v in data.items():
                    getattr(st, k).copy_(_t(v))

            ep_start = np.zeros((T, E), bool)
            ep_start[1:] = done[:-1] != 0
            want = old_returns.copy()
            for i in range(N):
                co.gae_single_pass(rewards[:, :, i], values[:, :, i], masks[:, :, i], want[:, :, i], ep_start, GAMMA, TAU)

            load()
            mom, mean, std = [x.clone() for x in eng.gae_moments(GAMMA, TAU)]
            got = st.returns.cpu().numpy()
            assert np.array_equal(_bits(got), _bits(want)), tag                # stale entries and row T included
            assert np.array_equal(_bits(got[T]), _bits(old_returns[T])), tag
            stale = np.broadcast_to(ep_start[:, :, None, None], (T, E, N, 1))
            assert np.array_equal(_bits(got[:-1][stale]), _bits(old_returns[:-1][stale])), tag
            for i in range(N):                                                  # the moments against numpy in fp64
                a = (want[:-1, :, i] - values[:-1, :, i]).astype(np.float32).astype(np.float64)
                m2 = ((a - a.mean()) ** 2).sum()
                assert float(mom[i, 0]) == T * E, tag
                assert abs(float(mean[i]) - a.mean()) <= 1e-12 * max(1.0, abs(a.mean())), tag
                assert abs(float(mom[i, 1]) - a.mean()) <= 1e-12 * max(1.0, abs(a.mean())), tag
                assert abs(float(mom[i, 2]) - m2) <= 1e-12 * m2, tag
                assert abs(float(std[i]) - np.sqrt(m2 / (a.size - 1))) <= 1e-12 * np.sqrt(m2 / (a.size - 1)), tag
            adv_ref = eng.adv_normalize(mean, std).clone()
            load()
            adv, mom_n, mean_n, std_n = eng.gae_normalize(GAMMA, TAU, out=adv_out)
            assert np.array_equal(_bits(st.returns.cpu().numpy()), _bits(got)), tag
            assert torch.equal(mom_n, mom) and torch.equal(mean_n, mean) and torch.equal(std_n, std), tag
            assert np.array_equal(_bits(adv.cpu().numpy()), _bits(adv_ref.cpu().numpy())), tag
            for _ in range(3):                                                  # run-to-run identical
                load()
                m3, mean3, std3 = eng.gae_moments(GAMMA, TAU)
                assert torch.equal(m3, mom) and torch.equal(mean3, mean) and torch.equal(std3, std), tag
                assert np.array_equal(_bits(st.returns.cpu().numpy()), _bits(got)), tag
