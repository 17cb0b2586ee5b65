"""CPU: the cross-play additions to the C ABI (the guard-pool fields of fa_policy_io, fa_match_*) have the layout the binding
assumes and refuse a NULL handle by name; the two pure functions of the evaluator; the CLI's --help."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fa():
    import emergent_multiagent_strategies_amd as m
    from emergent_multiagent_strategies_amd import build
    build.build()  # hipcc cross-compiles for gfx950 without a GPU
    return m


def test_policy_io_layout_matches_header(fa, tmp_path):
    """sizeof / offsetof from a C translation unit including the header == ctypes (the method of
    test_abi_cpu.test_struct_layout_matches_header): the guard-pool fields are appended, opp_attn stays where it was."""
    fields = ["opp_attn", "guard_pool", "guard_pool_size", "env_guard_strategy"]
    prog = ["#include <stdio.h>", "#include <stddef.h>", '#include "fortattack.h"', "int main(void){",
            'printf("size %zu\\n", sizeof(fa_policy_io));']
    for f in fields:
        prog.append('printf("%s %%zu\\n", offsetof(fa_policy_io, %s));' % (f, f))
    prog.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(fa._lib.PolicyIO)
    for f in fields:
        assert int(got[f]) == getattr(fa._lib.PolicyIO, f).offset, f
    # appended at the end: everything up to and including opp_attn keeps its offset
    assert fa._lib.PolicyIO.guard_pool.offset == fa._lib.PolicyIO.opp_attn.offset + 2 * C.sizeof(C.c_void_p)


def test_match_calls_refuse_a_null_handle_by_name(fa):
    lib = fa._lib.load()
    rem = C.c_int32(0)
    assert lib.fa_match_begin(None, None, 1, 1, None) < 0 and b"fa_match_begin" in lib.fa_last_error()
    assert lib.fa_match_latch(None, None) < 0 and b"fa_match_latch" in lib.fa_last_error()
    assert lib.fa_match_table(None, None, C.byref(rem), None) < 0 and b"fa_match_table" in lib.fa_last_error()


@pytest.mark.parametrize("E,off,ng,na", [(60, 0, 2, 3), (70, 0, 4, 3), (37, 5, 5, 5), (4096, 8192, 5, 5), (3, 0, 2, 2)])
def test_crossplay_cells_are_balanced(fa, E, off, ng, na):
    cell, gid, aid = fa.crossplay_cells(E, off, ng, na)
    for a in (cell, gid, aid):
        assert a.dtype == np.int32 and a.shape == (E,)
    assert np.array_equal(cell, (off + np.arange(E)) % (ng * na))
    assert np.array_equal(gid, cell // na) and np.array_equal(aid, cell % na)
    assert gid.max() < ng and aid.max() < na and cell.min() >= 0
    counts = np.bincount(cell, minlength=ng * na)
    assert set(counts) <= {E // (ng * na), -(-E // (ng * na))}
    assert counts.sum() == E


def test_crossplay_cells_of_shards_concatenate(fa):
    whole = fa.crossplay_cells(60, 0, 2, 3)
    a, b = fa.crossplay_cells(30, 0, 2, 3), fa.crossplay_cells(30, 30, 2, 3)
    for w, x, y in zip(whole, a, b):
        assert np.array_equal(w, np.concatenate([x, y]))
    # ... also where the shard size is no multiple of the cell count
    whole = fa.crossplay_cells(50, 0, 2, 3)
    a, b = fa.crossplay_cells(25, 0, 2, 3), fa.crossplay_cells(25, 25, 2, 3)
    assert np.array_equal(whole[0], np.concatenate([a[0], b[0]]))


def test_crossplay_rows_against_a_hand_written_block(fa):
    G, A = 2, 1
    # [latched envs, episodes, all dead, timeout, fort, alive_end g0 g1 a0, reward sums g0 g1 a0]
    raw = np.array([[2, 4, 1, 2, 1, 4, 2, 1, 8.0, -4.0, 6.0],
                    [0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0],
                    [1, 1, 0, 0, 1, 0, 1, 1, -1.5, 0.5, 3.0]])
    want = np.array([[0.25, 0.5, 0.75, 0.25, 1.5, 0.25, 0.5, 1.5],
                     [0, 0, 0, 0, 0, 0, 0, 0],
                     [0, 0, 0, 1, 1, 1, -0.5, 3.0]])
    got = fa.crossplay_rows(raw, G)
    assert got.shape == (3, 8) and np.array_equal(got, want)


def test_eval_cli_help_needs_no_gpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "eval_fortattack_amd.py"), "--help"], capture_output=True, text=True,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr
    for flag in ("--guard-load-dir", "--guard-ckpts", "--attacker-load-dir", "--attacker-ckpts", "--num-eval-episodes",
                 "--num-processes", "--num-guards", "--num-attackers", "--seed"):
        assert flag in r.stdout, flag
