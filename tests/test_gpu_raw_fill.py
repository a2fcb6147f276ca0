"""Fill-in from an untouched source entry (ref_lu_pipe.h, slip_fill_raw) on the device: the constructed cases of
tests/test_emu_raw_fill.py with their known counts, the widest golden (the memory path), 10teams (the lane path) and the
headline window, where the path has to carry most of the updates."""
import numpy as np
import pytest

import oracle_lib
import test_emu_raw_fill as T
from conftest import check_against_golden, load_case

pytestmark = pytest.mark.gpu

CASES = [(lambda r=r: T.case_widths_and_signs(r)) for r in T.RHO0] + list(T.SMALL_CASES) + [T.case_long_column, T.case_row_nearly_full]
IDS = ["widths_rho0_%d" % r for r in T.RHO0] + [c.__name__ for c in T.SMALL_CASES] + ["case_long_column", "case_row_nearly_full"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gpu_raw_fill_constructed(case):
    n, cols, want = case()
    T.check_constructed(None, n, cols, want, 8, 0, 0)


def test_gpu_raw_fill_constructed_few_workers():
    """two workers: columns wait long for their turn, sources arrive one frontier step at a time"""
    n, cols, want = T.case_widths_and_signs(-3)
    T.check_constructed(None, n, cols, want, 8, 2, 0)


def test_gpu_raw_fill_in_the_forward_solve():
    import slip_lu_amd as sl
    n, cols = T.base_matrix(-3, 0xF00DF00D, -0x1234567890ABCDEF)
    Ap, Ai, Alen, Alimbs = T.csc(n, cols)
    q = np.arange(n, dtype=np.int32)
    b = np.zeros(n, np.int64)
    b[1] = -(2 ** 35 + 7); b[6] = 5; b[15] = -3
    f = sl.Factorization(n, Ap, Ai, Alen, Alimbs, q, pivot=T.DIAGONAL)
    try:
        f.run(0)
        before = f.info()["raw_fills"]
        xlen, xlimbs = f.solve(np.sign(b).astype(np.int32), np.abs(b[b != 0]).astype(np.uint64))
        after = f.info()["raw_fills"]
    finally:
        f.close()
    want, _ = oracle_lib.factorize_and_solve(n, Ap, Ai, Alen, Alimbs, q, b, pivot=T.DIAGONAL)
    assert oracle_lib.bigints(xlen, xlimbs) == want
    assert after - before == 11, (before, after)      # rows 2..13 of L(:,1) but row 6 (tests/test_emu_raw_fill.py)


def _golden(name):
    import slip_lu_amd as sl
    entry, fix = load_case(name)
    res = sl.factorize(entry["n"], fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"], pivot=entry["pivot"], tol=entry["tol"],
                       kmax=entry["kmax"], limb_cap=entry["cap"])
    check_against_golden(entry, fix, res)
    return res["info"]


@pytest.mark.parametrize("name", ["de080285", "10teams"])
def test_gpu_raw_fill_goldens(name):
    """de080285: values of up to 407 limbs (the path through memory); 10teams: one-limb values (the lane)"""
    i = _golden(name)
    print(f"{name}: raw_fills {i['raw_fills']} of n_upd {i['n_upd']}")
    assert 0 < i["raw_fills"] <= i["n_upd"], i


def test_gpu_raw_fill_carries_the_headline_window():
    """C4: 10 647 of the 11 851 updates (89.8 %) have an untouched source and a zero target at pattern level; numerical
    cancellation can move a few rows, 0.8 leaves that room and fails if the heavy columns do not take the path"""
    i = _golden("C4_n100k_c64")
    print(f"C4 window: raw_fills {i['raw_fills']} of n_upd {i['n_upd']}")
    assert i["raw_fills"] >= 0.8 * i["n_upd"], i
