"""Solutions as multi-precision floats on the device: slip_hip_solution_to_mpfr against MPFR's recorded answers,
slip_hip_factor_solve_mpfr (plain, transposed, scaled) against the reference's rationals and the handle's own numerators through
the model of mpfr_set_q, integer solutions, a determinant beyond 256 digits, the handle's lifecycle."""
import pytest

from mpfr_helpers import (check_corpus, check_integer_solutions, check_lifecycle, check_reference_solutions,
                          check_reference_tsolutions, check_rejections, check_scale, check_wide_handle)

pytestmark = pytest.mark.gpu


def test_kernel_matches_mpfr_corpus():
    """the whole corpus, one call per (precision, mode), the operands above 8192 bits and the precision above 256 digits
    included; every path is taken"""
    total, paths = check_corpus(None)
    assert total == 5 * 28 * 12 * 8 + 5 * 6 * 2 and sum(paths) == total
    assert all(v > 0 for v in paths), paths


@pytest.mark.parametrize("name", ["solve_test_mat", "solve_gen_n40", "solve_10teams"])
def test_solve_mpfr_matches_reference(name):
    check_reference_solutions(None, name, nrhs=3)


@pytest.mark.parametrize("name", ["tsolve_test_mat", "tsolve_gen_n40", "tsolve_10teams"])
def test_solve_mpfr_transposed_matches_reference(name):
    check_reference_tsolutions(None, name, nrhs=3)


@pytest.mark.parametrize("name", ["solve_gen_n40", "solve_10teams"])
def test_integer_solutions_come_back_exactly(name):
    assert check_integer_solutions(None, name)[1] > 0       # the nonzero ones are long divisions


@pytest.mark.parametrize("name", ["solve_test_mat", "solve_10teams"])
def test_scale(name):
    check_scale(None, name)


def test_wide_determinant():
    """model6: det of more than 256 digits (the golden tests/test_gpu_check.py runs its memory path on)"""
    check_wide_handle(None, "model6")


def test_solve_mpfr_lifecycle():
    check_lifecycle(None, "solve_gen_n40")


def test_mpfr_rejects_bad_input():
    check_rejections(None, "solve_test_mat")
