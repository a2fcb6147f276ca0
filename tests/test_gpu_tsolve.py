"""The exact transposed solve on the MI355X (slip_hip_factor_solve_transpose: A(:,q)^T x = b on the resident factors, through
their transposed view) and its certificate (slip_hip_factor_check_transpose): the reference's own rationals of A^T x = b,
the CPU restatement on the explicitly transposed matrix, the duality with the plain solve on complete goldens across the
pivot rules and the limb range, the certificate's verdicts and rejections, and the handle's lifecycle."""
import pytest

from tsolve_helpers import (check_cpu_restatement, check_duality, check_duplicates, check_lifecycle, check_reference_tsolve,
                            check_rejections, check_verdicts)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,nrhs,kw", [
    ("tsolve_test_mat", 1, {}), ("tsolve_gen_n40", 3, {}), ("tsolve_10teams", 1, {}),
    ("tsolve_10teams", 16, {}),                                  # one worker per right-hand side
    ("tsolve_gen_n40", 2, dict(workers=1)),                      # one worker takes the right-hand sides in turn
    ("tsolve_10teams", 1, dict(workers=3, waves=4)), ("tsolve_gen_n40", 1, dict(waves=1))])
def test_gpu_tsolve_matches_reference(name, nrhs, kw):
    check_reference_tsolve(None, name, nrhs=nrhs, **kw)


def test_gpu_tsolve_cpu_restatement_and_residual():
    check_cpu_restatement(None)


@pytest.mark.parametrize("name", ["test_mat", "test_mat_p0", "test_mat_p1", "test_mat_p2", "test_mat_p4", "test_mat_p5",
                                  "10teams_p5", "prob159", "rl5934", "rail4284", "de080285", "NSR8K"])
def test_gpu_tsolve_duality(name):
    check_duality(None, name)


@pytest.mark.parametrize("name", ["test_mat", "10teams"])
def test_gpu_check_transpose_verdicts(name):
    check_verdicts(None, name)


def test_gpu_check_transpose_keeps_the_last_duplicate():
    check_duplicates(None)


def test_gpu_transpose_rejects_bad_input():
    check_rejections(None)


@pytest.mark.parametrize("name", ["solve_gen_n40", "solve_10teams"])
def test_gpu_tsolve_lifecycle(name):
    check_lifecycle(None, name)
