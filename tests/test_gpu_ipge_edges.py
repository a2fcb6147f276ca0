"""The column update at every edge of its width classes on the device: the built cases of tests/ipge_edge_helpers.py (their
intent is asserted in tests/test_emu_ipge_edges.py), each against oracle_lib.factorize bit for bit and against the dense
fraction-free elimination in Python integers."""
import numpy as np
import pytest

import ipge_edge_helpers as H
from test_emu_batch_commit import FACTOR_KEYS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", H.cases_of("ABCD"))
def test_gpu_ipge_edges(case):
    H.check_intent(case)
    H.check_case(None, case, 8, 0, 0)


@pytest.mark.parametrize("case", H.cases_of("AC"))
def test_gpu_ipge_edges_few_workers(case):
    """two workers: columns wait long for their turn, sources arrive one frontier step at a time"""
    H.check_case(None, case, 8, 2, 0)


@pytest.mark.parametrize("case", H.cases_of("ABD", one_limb=True))
def test_gpu_ipge_edges_chain_engine_on_and_off(case):
    """one-limb columns: with debug_flags 0 the committer's chain engine may carry the column, with 8 the worker's sweep
    does; the same bytes both ways"""
    a = H.check_case(None, case, 8, 0, 0, debug_flags=0)
    b = H.check_case(None, case, 8, 0, 0, debug_flags=8)
    for k in FACTOR_KEYS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize("name", H.E_CASES)
def test_gpu_ipge_edges_in_the_solve(name):
    """Family E: the forward substitution is the same sweep; numerators against Fraction arithmetic"""
    case = H.case_named("B", name)
    H.solve_check(None, case, H.edge_rhs(case, 2), 8, 0, 0)
