"""CPU: what the C ABI answers to null arguments, export by export, and that a variant library of tools/build_variant.py loads.

Every export called with null pointers and zero scalars returns the code and leaves the message recorded in
tests/golden/api_null_errors.json (taken from the library before its host layer was split per subsystem: the checks that
open an export moved into one helper, their answers did not change).  Nothing here needs a device: each of these calls is
refused before it touches one."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "api_null_errors.json")
# not swept: covered by test_abi_cpu.py, nothing to refuse (void / no arguments / a null is fine), or no error path
LEFT_OUT = {"fa_config_default", "fa_destroy", "fa_last_error", "fa_rccl_comm_destroy", "fa_rccl_available", "fa_rccl_library",
            "fa_step_variant", "fa_policy_variant", "fa_policy_weight_floats", "fa_policy_plain_floats",
            "fa_policy_weight_t_floats", "fa_ppo_grad_floats", "fa_adam_scratch_floats"}
SETS_NO_MESSAGE = {"fa_num_agents", "fa_num_envs"}


@pytest.fixture(scope="module")
def fa():
    import emergent_multiagent_strategies_amd as m
    from emergent_multiagent_strategies_amd import build
    build.build()
    return m


def null_sweep(fa):
    """{export: [return code, message]} of every swept export called with all-zero arguments."""
    lib = fa._lib.load()
    out = {}
    for name, (_, argtypes) in sorted(fa._lib.EXPORTS.items()):
        if name in LEFT_OUT:
            continue
        lib.fa_config_default(None)                  # a known message, so that an export that sets none shows
        marker = lib.fa_last_error()
        rc = getattr(lib, name)(*[t() for t in argtypes])   # t(): a null pointer / a zero scalar
        msg = lib.fa_last_error()
        out[name] = [int(rc), None if msg == marker else msg.decode()]
    return out


def test_null_arguments_return_the_recorded_errors(fa):
    want = json.load(open(GOLDEN))
    assert len(want) == 49 and sorted(want) == sorted(set(fa._lib.EXPORTS) - LEFT_OUT)
    got = null_sweep(fa)
    for name in sorted(want):
        assert got[name] == want[name], name
        assert got[name][0] == -1 and (got[name][1] is None) == (name in SETS_NO_MESSAGE), name


def test_a_variant_library_loads(fa):
    """tools/build_variant.py on top of the product build (fa_fold.hip: the cheapest translation unit to recompile): the result
    loads and resolves every export -- the tool links the same translation units as build.py."""
    name = "abi_load_check"
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "build_variant.py"), name, "fa_fold.hip"],
                                  text=True).strip().splitlines()[-1]
    try:
        assert os.path.basename(out) == "lib_%s.so" % name
        lib = C.CDLL(out)
        for sym in fa._lib.EXPORTS:
            assert hasattr(lib, sym), sym
    finally:
        os.remove(out)
