"""The pivot rules against the compiled reference on the pivot-edge corpus (tests/pivot_corpus.py): the CPU restatement
(oracle/liboracle.so) and the kernel source on the CPU emulation (tests/emu/libslip_emu.so).

Bit-exact: pinv and the SHA-256 over L, U, rho decide whether the same pivot rows were chosen -- the exact solve check
cannot, since any pivot row gives a valid REF LU."""
import os
import subprocess
import sys

import pytest

import oracle_lib
import pivot_corpus as pc
from conftest import ROOT

EMU = os.path.join(ROOT, "tests", "emu", "libslip_emu.so")


@pytest.mark.parametrize("pivot", range(6))
def test_oracle_matches_reference_on_pivot_corpus(pivot):
    bad = []
    for run in pc.runs(pivots=(pivot,)):
        n, Ap, Ai, Alen, Alimbs, q = pc.matrix(run["matrix"])
        res = oracle_lib.factorize(n, Ap, Ai, Alen, Alimbs, q, pivot=pivot, tol=run["tol"])
        try:
            pc.check_run(run, res)
        except AssertionError as e:
            bad.append((pc.label(run), str(e)[:80]))
    assert not bad, "%d of %d runs differ from the reference: %s" % (len(bad), len(pc.runs(pivots=(pivot,))), bad[:8])


RANDOM = ["random%02d" % i for i in range(20)]
CRAFTED = ["crafted00", "crafted04", "singular0"]


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "libslip_emu.so"])
    return EMU


# The kernel decides the diagonal preference at five places; the shapes are picked so that each of them decides
# scheme-4 columns whose largest candidate is negative (established with the emulator's trace build, -DSLIP_EMU_TRACE):
#   (1, 1, 8)  one worker, no committer: the early commit's search (diag_rule after search_publish)
#   (2, 3, 1)  no early commit: the complete path (diag_rule after the full search)
#   (2, 5, 8)  candidates-only packages: the committer's batch step and its serial step
#   (2, 6, 0)  full packages: the committer's chain engine
@pytest.mark.parametrize("waves,workers,flags,seed", [(1, 1, 8, 1), (2, 3, 1, 2), (2, 5, 8, 3), (2, 6, 0, 1), (2, 3, 0, 4)])
def test_emulated_kernel_matches_reference_on_pivot_corpus(emu_lib, waves, workers, flags, seed):
    """the kernel source on the CPU emulation: every scheme on the small random matrices, scheme 4 (tol 0.5) on
    a few crafted ones; several schedules"""
    import ctypes
    import slip_lu_amd as sl
    lib = ctypes.CDLL(emu_lib)
    lib.slip_emu_set_seed.argtypes = [ctypes.c_ulonglong]
    lib.slip_emu_set_seed(seed)
    todo = pc.runs(matrices=RANDOM) + [r for r in pc.runs(pivots=(4,), matrices=CRAFTED) if r["tol"] == 0.5]
    bad, info = [], dict(committer_commits=0, engine_commits=0)
    for run in todo:
        n, Ap, Ai, Alen, Alimbs, q = pc.matrix(run["matrix"])
        res = sl.factorize(n, Ap, Ai, Alen, Alimbs, q, pivot=run["pivot"], tol=run["tol"], waves=waves, workers=workers,
                           lib_path=emu_lib, check=False, debug_flags=flags)
        for k in info:
            info[k] += res["info"][k]
        try:
            pc.check_run(run, res)
        except AssertionError as e:
            bad.append((pc.label(run), str(e)[:80]))
    assert not bad, "%d of %d runs differ from the reference: %s" % (len(bad), len(todo), bad[:8])
    if (workers, flags) == (5, 8):
        assert info["committer_commits"] > 0 and info["engine_commits"] == 0, info
    if (workers, flags) == (6, 0):
        assert info["engine_commits"] > 0, info
