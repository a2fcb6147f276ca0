"""Bounds in the exact selections on the MI355X (slip_hip_ratio_test_bounded, slip_hip_bound_test and their fused forms on a
handle), against Python fractions in the direct formulation: the reduction to the unbounded ratio test, every width class of
the form pass, signs, zeros and sides, unreduced ties, the launch geometry up to several workgroups, the bound test, handles
on complete goldens (de080285 reaches the memory path of the form pass on real data; one handle has a negative determinant)
and every rejected input."""
import pytest

from bound_helpers import (check_bound_test, check_geometry, check_golden, check_negative_det, check_reduction, check_reduction_on_handle,
                           check_rejections, check_signs_and_sides, check_ties, check_width_classes)

pytestmark = pytest.mark.gpu


def test_gpu_bound_reduces_to_the_ratio_test():
    check_reduction(None)


def test_gpu_bound_reduces_to_the_ratio_test_on_a_handle():
    check_reduction_on_handle(None, "test_mat")


def test_gpu_bound_width_classes():
    check_width_classes(None)


def test_gpu_bound_signs_zeros_sides():
    check_signs_and_sides(None)


def test_gpu_bound_unreduced_ties():
    check_ties(None)


def test_gpu_bound_geometry():
    check_geometry(None, (1, 63, 64, 65, 130, 600))


def test_gpu_bound_test():
    check_bound_test(None)


@pytest.mark.parametrize("name", ["test_mat", "gen_n40", "10teams", "prob159", "de080285"])
def test_gpu_bound_on_handles(name):
    check_golden(None, name, memory_path=name == "de080285")


def test_gpu_bound_negative_determinant():
    check_negative_det(None)


def test_gpu_bound_rejects_bad_input():
    check_rejections(None)
