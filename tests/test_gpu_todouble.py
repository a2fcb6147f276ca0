"""Solutions as doubles on the device: slip_hip_solution_to_double against GMP's recorded answers, slip_hip_factor_solve_double
(plain, transposed, scaled) against the reference's rationals and the handle's own numerators, integer solutions, a determinant
beyond 256 digits, the handle's lifecycle."""
import pytest

from todouble_helpers import (check_corpus, check_integer_solutions, check_lifecycle, check_reference_solutions,
                              check_reference_tsolutions, check_rejections, check_scale, check_wide_handle)

pytestmark = pytest.mark.gpu


def test_kernel_matches_gmp_corpus():
    """the whole corpus in one call, the operands above 8192 bits included"""
    assert check_corpus(None) >= 25 * 24


@pytest.mark.parametrize("name", ["solve_test_mat", "solve_gen_n40", "solve_10teams"])
def test_solve_double_matches_reference(name):
    check_reference_solutions(None, name, nrhs=3)


@pytest.mark.parametrize("name", ["tsolve_test_mat", "tsolve_gen_n40", "tsolve_10teams"])
def test_solve_double_transposed_matches_reference(name):
    check_reference_tsolutions(None, name, nrhs=3)


@pytest.mark.parametrize("name", ["solve_gen_n40", "solve_10teams"])
def test_integer_solutions_come_back_exactly(name):
    assert check_integer_solutions(None, name) > 0          # they do take the wave pass


@pytest.mark.parametrize("name", ["solve_test_mat", "solve_10teams"])
def test_scale(name):
    check_scale(None, name)


def test_wide_determinant():
    """model6: det of more than 256 digits (the golden tests/test_gpu_check.py runs its memory path on)"""
    check_wide_handle(None, "model6")


def test_solve_double_lifecycle():
    check_lifecycle(None, "solve_gen_n40")


def test_solution_to_double_rejects_bad_input():
    check_rejections(None)
