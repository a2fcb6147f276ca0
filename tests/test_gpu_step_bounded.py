"""The bounded exact simplex step on the MI355X (slip_hip_step_bounded, slip_hip_factor_step_bounded), against Python integers
and fractions in the direct formulation on the true values: the three moves with ties, both sides and x outside its bounds up
to several waves a problem, every width class of slip_bstep_kernel on both sides of its edge and the memory path, the
reduction to Factorization.step, the end-to-end proof of a pivot and of a flip, inexact divisions, more than one staging
group, the lifecycle of a handle and every refused input."""
import pytest

from step_bounded_helpers import (check_groups, check_inexact, check_lifecycle, check_moves, check_proof, check_reduction,
                                  check_rejections, check_width_classes)

pytestmark = pytest.mark.gpu


def test_gpu_step_bounded_moves():
    check_moves(None, (1, 63, 64, 65, 130))


def test_gpu_step_bounded_width_classes():
    check_width_classes(None, sizes=(4, 64, 128, 192, 256), memory=300)


@pytest.mark.parametrize("name", ["test_mat", "gen_n40"])
def test_gpu_step_bounded_reduction(name):
    check_reduction(None, name)


@pytest.mark.parametrize("name", ["test_mat", "gen_n40"])
def test_gpu_step_bounded_proof(name):
    check_proof(None, name, negative_det=name == "test_mat")


def test_gpu_step_bounded_inexact():
    check_inexact(None)


def test_gpu_step_bounded_groups():
    check_groups(None, n=130)


def test_gpu_step_bounded_lifecycle():
    check_lifecycle(None, "gen_n40")


def test_gpu_step_bounded_rejects_bad_input():
    check_rejections(None)
