"""The exact ratio test on the MI355X (slip_hip_ratio_test, slip_hip_factor_ratio_test), against Python fractions: every width
class of the exact comparison, unreduced ties, signs and zeros, the launch geometry up to several workgroups, integer vectors
without denominators, handles on complete goldens (de080285 reaches the memory path on real data; one handle has a negative
determinant), the lifecycle of a handle and every rejected input."""
import pytest

from ratio_helpers import (check_geometry, check_golden, check_lifecycle, check_negative_det, check_no_denominators, check_rejections,
                           check_signs_and_zeros, check_ties, check_width_classes)

pytestmark = pytest.mark.gpu


def test_gpu_ratio_width_classes():
    check_width_classes(None)


def test_gpu_ratio_unreduced_ties():
    check_ties(None)


def test_gpu_ratio_signs_and_zeros():
    check_signs_and_zeros(None)


def test_gpu_ratio_geometry():
    check_geometry(None, (1, 63, 64, 65, 130, 600))


def test_gpu_ratio_without_denominators():
    check_no_denominators(None)


@pytest.mark.parametrize("name", ["test_mat", "gen_n40", "10teams", "prob159", "de080285"])
def test_gpu_ratio_on_handles(name):
    check_golden(None, name, memory_path=name == "de080285")


def test_gpu_ratio_negative_determinant():
    check_negative_det(None)


def test_gpu_ratio_lifecycle():
    check_lifecycle(None)


def test_gpu_ratio_rejects_bad_input():
    check_rejections(None)
