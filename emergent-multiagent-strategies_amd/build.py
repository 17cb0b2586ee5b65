"""Compile the HIP engine for gfx950 (in-tree, so the .so travels with the repo)."""
import os
import shutil
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(CSRC, "libfortattack_hip.so")
# FA_LIBRARY: load another build of the same C ABI instead (the variant libraries of tools/build_variant.py -- the
# experiment step kernels' parity tests, A/B runs); never built or rebuilt from here
if os.environ.get("FA_LIBRARY"):
    LIB = os.path.abspath(os.environ["FA_LIBRARY"])
OBJ = os.path.join(CSRC, "_obj")            # objects + assembly of the last build (git-ignored)
SOURCES = ["fa_step_pipe.hip", "fa_step_classic.hip", "fa_collect.hip", "fa_policy.hip", "fa_match.hip", "fa_render.hip", "fa_behaviour.hip", "fa_attend.hip", "fa_train.hip", "fa_train_dw.hip", "fa_fold.hip", "fa_rccl.hip", "fa_api.hip"]
# -ffp-contract=off: the fp64 step must evaluate every operation as the reference does
# (no fused multiply-add); no -ffast-math for the same reason.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared"]


def hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def needs_build():
    if os.environ.get("FA_LIBRARY"):
        return False
    if not os.path.isfile(LIB):
        return True
    import glob
    deps = [os.path.join(CSRC, f) for f in SOURCES] + [os.path.join(ROOT, "include", "fortattack.h")]
    deps += glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "experiments", "*.h"))
    return any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps)


def _load_mod(fname):
    import importlib.util           # by path: this file is also loaded stand-alone (__graft_entry__.build)
    spec = importlib.util.spec_from_file_location("_fa_" + fname[:-3], os.path.join(os.path.dirname(os.path.abspath(__file__)), fname))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _load_lint():
    return _load_mod("isa_lint.py")


def _compile_one(src, verbose):
    """One translation unit -> object file, plus its gfx950 assembly through isa_lint (the same flags: the same code)."""
    isa_lint = _load_lint()
    base = os.path.join(OBJ, os.path.splitext(src)[0])
    common = [hipcc()] + [f for f in FLAGS if f != "-shared"] + ["-I", os.path.join(ROOT, "include")]
    cmd = common + ["-c", os.path.join(CSRC, src), "-o", base + ".o"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    subprocess.check_call(common + ["-S", "--cuda-device-only", os.path.join(CSRC, src), "-o", base + ".s"])
    bad = isa_lint.lint(base + ".s")
    if bad:
        raise RuntimeError("isa_lint: %s has %d vector instruction(s) ahead of an exec restore (a misplaced live-range "
                           "split: lanes that skipped the region lose the value), first: %s %s line %d: %s"
                           % (src, len(bad), bad[0][0], bad[0][1], bad[0][2][0], bad[0][2][1]))
    return base + ".o"


def build(force=False, verbose=False):
    if os.environ.get("FA_LIBRARY") or (not force and not needs_build()):
        return LIB
    from concurrent.futures import ThreadPoolExecutor
    os.makedirs(OBJ, exist_ok=True)
    with ThreadPoolExecutor(max_workers=4) as pool:
        objs = list(pool.map(lambda f: _compile_one(f, verbose), SOURCES))
    # The issue model of the pipelined step kernel, read off this build's assembly (bench.py: roofline.secondary), and its
    # regression gate -- FLAT stores, spill reloads in the critical step loops, instruction count of wave 0's loop -- BEFORE the
    # link, so that a failed gate leaves no library behind that a second, non-forced build() would accept.  The gate is a
    # performance heuristic tied to one compiler version (hipcc 7.2): FA_ISA_GATE=0 turns its findings into warnings (the
    # correctness lint, isa_lint, stays fatal).  The model goes to the git-ignored _obj/; the tracked csrc/fa_isa_model.json is
    # only rewritten on request (FA_ISA_REFRESH=1 or `python isa_model.py --refresh`; tests/test_isa_lint_cpu.py keeps the two equal).
    isa_model = _load_mod("isa_model.py")
    m = isa_model.write(os.path.join(OBJ, "fa_step_pipe.s"), os.path.join(OBJ, "fa_isa_model.json"))
    if os.environ.get("FA_ISA_REFRESH") == "1":
        isa_model.write(os.path.join(OBJ, "fa_step_pipe.s"))
    bad = isa_model.check(m)
    if bad:
        msg = "isa_model: the shipped step-kernel instantiations regressed: " + "; ".join(bad)
        if os.environ.get("FA_ISA_GATE", "1") == "0":
            import warnings
            warnings.warn(msg + "  (FA_ISA_GATE=0: building anyway)")
        else:
            if os.path.isfile(LIB):
                os.remove(LIB)
            raise RuntimeError(msg + "  (FA_ISA_GATE=0 builds anyway)")
    cmd = [hipcc(), "--offload-arch=gfx950", "-fPIC", "-shared"] + objs + ["-o", LIB]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    print(build(force=True, verbose=True))
