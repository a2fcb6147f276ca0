"""Solutions as reduced fractions on the device: slip_hip_solution_to_rational against GMP's recorded canonical forms,
slip_hip_factor_solve_rational (plain, transposed, scaled) against the reference's rationals and the handle's own numerators,
integer solutions, a determinant beyond 256 digits, the handle's lifecycle, and the round trip through the exact check."""
import pytest

from rational_helpers import (check_certificate, check_corpus, check_integer_solutions, check_lifecycle, check_reference_solutions,
                              check_reference_tsolutions, check_rejections, check_scale, check_wide_handle)

pytestmark = pytest.mark.gpu


def test_kernel_matches_gmp_corpus():
    """the whole corpus in one call; each of the kernel's four paths settles some of it"""
    paths = check_corpus(None)
    assert all(p > 0 for p in paths), paths


@pytest.mark.parametrize("name", ["solve_test_mat", "solve_gen_n40", "solve_10teams"])
def test_solve_rational_matches_reference(name):
    check_reference_solutions(None, name, nrhs=3)


@pytest.mark.parametrize("name", ["tsolve_test_mat", "tsolve_gen_n40", "tsolve_10teams"])
def test_solve_rational_transposed_matches_reference(name):
    check_reference_tsolutions(None, name, nrhs=3)


@pytest.mark.parametrize("name", ["solve_gen_n40", "solve_10teams"])
def test_integer_solutions_come_back_over_one(name):
    check_integer_solutions(None, name)


@pytest.mark.parametrize("name", ["solve_test_mat", "solve_10teams"])
def test_scale(name):
    check_scale(None, name)


def test_wide_determinant():
    """model6: det of more than 256 digits, the kernel's memory class"""
    check_wide_handle(None, "model6")


def test_solve_rational_lifecycle():
    check_lifecycle(None, "solve_gen_n40")


def test_solution_to_rational_rejects_bad_input():
    check_rejections(None)


def test_reduced_fractions_pass_the_exact_check():
    check_certificate(None, "solve_gen_n40", nrhs=3)
