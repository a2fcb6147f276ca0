"""The rewind to column K (slip_hip_factor_rewind) and the replacement of a column of the resident A
(slip_hip_factor_replace_column) on the MI355X, against the CPU restatement on the matrix as it stands and the goldens.
Default workers: the committer and its chain engine start from a rewound frontier; once with one worker."""
import pytest

from update_helpers import (check_certificate, check_q_tail, check_refusals, check_replace, check_replace_ahead,
                            check_rewind_equals_run, check_rewind_then_run, check_sequence, check_singular_repaired,
                            check_storage_bound)

pytestmark = pytest.mark.gpu

TEAMS_KS = sorted(set(range(0, 178, 16)) | {0, 1, 176, 177})


@pytest.mark.parametrize("name,pivot,Ks,kw", [
    ("gen_n40", 0, None, {}), ("gen_n40", 1, None, {}), ("gen_n40", 3, None, {}), ("gen_n40", 5, None, {}),
    ("10teams", 3, TEAMS_KS, {}), ("gen_n40_pm1", 3, range(0, 41, 4), {}), ("test_mat", 3, None, {}),
    ("gen_n40", 3, range(0, 41, 3), dict(workers=1))])
def test_gpu_rewind_equals_run_to_K(name, pivot, Ks, kw):
    contested = check_rewind_equals_run(None, name, pivot, Ks, **kw)
    if name in ("gen_n40", "10teams") and pivot == 3:
        assert contested > 0            # positions the undo writes twice: the smallest column has to win there


@pytest.mark.parametrize("name,K,kw", [("test_mat", 4, {}), ("gen_n40", 11, {}), ("gen_n40_pm1", 29, {}), ("10teams", 60, {}),
                                       ("10teams", 171, dict(workers=1))])
def test_gpu_rewind_then_run_is_the_golden(name, K, kw):
    check_rewind_then_run(None, name, K, **kw)


@pytest.mark.parametrize("name", ["gen_n40", "10teams"])
@pytest.mark.parametrize("where,kind", [("first", "more"), ("middle", "fewer"), ("last", "single"), ("middle", "wide"),
                                        ("first", "dup"), ("last", "hizero"), ("middle", "single"), ("last", "more"),
                                        ("first", "wide")])
def test_gpu_replace_column_against_oracle(name, where, kind):
    check_replace(None, name, where, kind)


def test_gpu_replace_column_one_worker():
    check_replace(None, "gen_n40", "middle", "wide", workers=1)


@pytest.mark.parametrize("name", ["gen_n40", "10teams"])
def test_gpu_replace_ahead_of_the_frontier(name):
    check_replace_ahead(None, name)


def test_gpu_replacement_sequence():
    check_sequence(None, "gen_n40", steps=12)


def test_gpu_storage_bound():
    check_storage_bound(None, "test_mat", steps=64)


@pytest.mark.parametrize("name", ["gen_n40", "10teams"])
def test_gpu_singular_and_repaired(name):
    check_singular_repaired(None, name)


@pytest.mark.parametrize("name", ["gen_n40", "10teams"])
def test_gpu_certificate_sees_the_new_matrix(name):
    check_certificate(None, name)


@pytest.mark.parametrize("name", ["gen_n40", "10teams"])
def test_gpu_q_tail(name):
    check_q_tail(None, name)


def test_gpu_refusals():
    check_refusals(None, "test_mat")
