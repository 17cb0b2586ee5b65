"""GPU (a handle needs a device; nothing here launches a kernel): the state errors of the C ABI, text for text.

The checks that open an export -- null handle, bound storage, device -- are one helper (csrc/fa_env.h) and every subsystem's
exports live beside its kernels.  The strings below are the literals of the source before that move: an export that needs a
storage says so before one is bound, the match exports refuse a handle without counters, and latch / table / chunk / state
refuse to run before their begin.  (test_gpu_behaviour.py, test_gpu_crossplay.py and test_gpu_parity.py check a word of some
of these messages; here it is the whole text and the code.)"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

FA_ERR_INVALID, FA_ERR_STATE = -1, -3


@pytest.fixture(scope="module")
def fa():
    import emergent_multiagent_strategies_amd as m
    m._lib.load()
    return m


def _refused(lib, name, h, args, code, text):
    rc = getattr(lib, name)(h, *args)
    msg = lib.fa_last_error().decode()
    assert (rc, msg) == (code, text), name


def test_state_errors_keep_their_texts(fa):
    lib = fa._lib.load()
    eng = fa.BatchedFortAttack(2, 1, 1, 4)
    bare = fa.BatchedFortAttack(2, 1, 1, 4, track_counters=False)
    buf = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = C.c_void_p(buf.data_ptr())      # passes the null checks; every call below is refused before it is read
    io = fa._lib.PolicyIO()
    needs_storage = [                   # (export, its arguments after the handle, the export named by the message)
        ("fa_collect_step", (0, 1, None), "fa_collect_rollout"),
        ("fa_collect_rollout", (0, 1, 1, None), None),
        ("fa_collect_reset", (None,), None),
        ("fa_gae", (0.99, 0.95, None), None),
        ("fa_gae_moments", (0.99, 0.95, p, p, p, None), None),
        ("fa_gae_normalize", (0.99, 0.95, p, p, p, p, None), None),
        ("fa_adv_moments_onepass", (p, p, p, None), None),
        ("fa_adv_stats", (0, None, p, None), None),
        ("fa_adv_mean_std", (p, p, None), None),
        ("fa_adv_moments", (p, None), None),
        ("fa_adv_merge_normalize", (p, 1, p, p, p, None), None),
        ("fa_adv_normalize", (p, p, p, None), None),
        ("fa_after_update", (None,), None),
        ("fa_collect_act", (0, C.byref(io), None), None),
        ("fa_behaviour_chunk", (None,), None),
    ]
    for name, args, who in needs_storage:
        _refused(lib, name, eng._h, args, FA_ERR_STATE, "%s: no storage bound" % (who or name))
    # this one looks at `world` before the storage
    _refused(lib, "fa_adv_merge_normalize", eng._h, (p, 0, p, p, p, None), FA_ERR_INVALID,
             "fa_adv_merge_normalize: world must be >= 1")

    for name, args in (("fa_match_begin", (p, 1, 1, None)), ("fa_match_latch", (None,)), ("fa_match_table", (p, None, None))):
        _refused(lib, name, bare._h, args, FA_ERR_STATE, "%s: the handle was created with track_counters = 0" % name)

    eng.bind_storage(fa.JointRolloutStorage(2, 2, 2, device="cuda"))
    _refused(lib, "fa_match_latch", eng._h, (None,), FA_ERR_STATE, "fa_match_latch: no match begun (fa_match_begin)")
    _refused(lib, "fa_match_table", eng._h, (p, None, None), FA_ERR_STATE, "fa_match_table: no match begun (fa_match_begin)")
    _refused(lib, "fa_behaviour_chunk", eng._h, (None,), FA_ERR_STATE, "fa_behaviour_chunk: no record begun (fa_behaviour_begin)")
    _refused(lib, "fa_behaviour_state", eng._h, (None, None), FA_ERR_STATE,
             "fa_behaviour_state: no record begun (fa_behaviour_begin)")
    # ... and through the binding: the text reaches FaError whole
    with pytest.raises(fa.FaError, match=r"fa_gae failed \(-3\): fa_gae: no storage bound$"):
        bare.gae()
