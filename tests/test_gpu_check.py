"""The exact solution check on the MI355X (slip_hip_factor_check, slip_hip_check_solution): the solve's own numerators pass
on the complete goldens (the memory path included), perturbed numerators are reported exactly where the Python-integer
residual says, the reference's rationals pass the standalone check, and rejected input is rejected."""
import numpy as np
import pytest

import oracle_lib
from check_helpers import (check_clean, check_duplicates, check_error_paths, check_perturbations, check_reference_rationals,
                           check_wide, factor_and_solve, rhs_pair, slab)
from conftest import load_case

pytestmark = pytest.mark.gpu


def _digits(lens, limbs):
    """32-bit digit count of every entry of a limb slab"""
    out, o = np.zeros(len(lens), np.int64), 0
    for t, l in enumerate(lens):
        a = abs(int(l))
        if a:
            top = int(limbs[o + a - 1])
            out[t] = 2 * a - (1 if top >> 32 == 0 else 0)
        o += a
    return out


def _max_width(fix, q, n, nrhs, xlen, xlimbs):
    """the largest W = max(|a| + |x|) + 1 over the (row, rhs) pairs of the A(:,q) x part of the check"""
    adig = _digits(fix["Alen"], fix["Alimbs"])
    xdig = _digits(xlen, xlimbs).reshape(nrhs, n)
    colmax = np.zeros(n, np.int64)                    # widest entry of each column of A
    for j in range(n):
        s, e = int(fix["Ap"][j]), int(fix["Ap"][j + 1])
        if e > s:
            colmax[j] = adig[s:e].max()
    pos_of = np.empty(n, np.int64)
    pos_of[np.asarray(q, np.int64)] = np.arange(n)
    return int((colmax[None, :] + xdig[:, pos_of]).max()) + 1


@pytest.mark.parametrize("name", ["test_mat", "10teams", "prob159", "rl5934", "rail4284", "model6", "de080285", "NSR8K"])
def test_gpu_check_of_clean_solves(name):
    import slip_lu_amd as sl
    _, fix = load_case(name)
    n, q = len(fix["q"]), fix["q"]
    f = sl.Factorization(n, fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], q)
    try:
        f.run(0)
        b0 = oracle_lib.solve_rhs(n)
        bs = [[int(v) for v in b0], [(int(v) * 3 + 1) * (2 ** 90 + 17) for v in b0]]      # the second one multi-limb
        blen, blimbs = slab([v for b in bs for v in b])
        xlen, xlimbs = f.solve(blen, blimbs, nrhs=2)
        for nrhs in (1, 2):
            xl = xlen[:nrhs * n]
            nl = int(np.abs(xl.astype(np.int64)).sum())
            bl = blen[:nrhs * n]
            ok, first, bad = f.check(bl, blimbs[:int(np.abs(bl.astype(np.int64)).sum())], xl, xlimbs[:nl], nrhs=nrhs)
            assert ok, (name, nrhs, first, bad)
            assert list(first) == [-1] * nrhs and list(bad) == [0] * nrhs
        if name in ("model6", "de080285"):
            assert _max_width(fix, q, n, 2, xlen, xlimbs) > 256, "the memory path (W > 256 digits) was not reached"
    finally:
        f.close()


@pytest.mark.parametrize("name", ["10teams", "de080285"])
def test_gpu_check_finds_perturbations(name):
    _, fix = load_case(name)
    n, Ap, Ai, Alen, Alimbs, q = len(fix["q"]), fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"]
    bs = rhs_pair(n)
    f, x, det = factor_and_solve(None, n, Ap, Ai, Alen, Alimbs, q, bs)
    try:
        check_clean(f, n, x, bs)
        check_perturbations(f, n, Ap, Ai, Alen, Alimbs, q, x, det, bs)
    finally:
        f.close()


@pytest.mark.parametrize("name", ["solve_test_mat", "solve_gen_n40", "solve_10teams"])
def test_gpu_check_of_reference_rationals(name):
    check_reference_rationals(None, name)


@pytest.mark.parametrize("ylimbs", [150, 400])
def test_gpu_check_wide_path(ylimbs):
    check_wide(None, 30, ylimbs, 8, ylimbs)


def test_gpu_check_keeps_the_last_duplicate():
    check_duplicates(None)


def test_gpu_check_rejects_bad_input():
    check_error_paths(None)
