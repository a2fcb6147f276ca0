"""The exact pivot update on the MI355X (slip_hip_pivot_update, slip_hip_factor_solve_update, slip_hip_factor_step), against
Python integers and fractions: every width class of the form pass and every kind of divisor, signs, zeros and the form without
a division, inexact divisions of every path, placement and the launch geometry up to several workgroups, steps on complete
goldens (de080285 reaches the memory path on real data) with the end-to-end proof against the replaced basis and the dual
form, the lifecycle of a handle and every rejected input."""
import pytest

from pivot_update_helpers import (check_geometry, check_golden, check_inexact, check_lane_carry, check_lifecycle, check_rejections,
                                  check_signs_and_zeros, check_width_classes)

pytestmark = pytest.mark.gpu


def test_gpu_pivot_update_width_classes():
    check_width_classes(None)


def test_gpu_pivot_update_signs_and_zeros():
    check_signs_and_zeros(None)


def test_gpu_pivot_update_lane_carry():
    check_lane_carry(None)


def test_gpu_pivot_update_inexact():
    check_inexact(None)


def test_gpu_pivot_update_geometry():
    check_geometry(None, (1, 63, 64, 65, 130, 600))


@pytest.mark.parametrize("name", ["test_mat", "gen_n40", "10teams", "prob159", "de080285"])
def test_gpu_step_on_handles(name):
    # (de080285: one orientation and no second substitution; one of its right-hand sides takes 0.6 s)
    wide = name == "de080285"
    check_golden(None, name, memory_path=wide, transposes=(False,) if wide else (False, True), proof=name in ("test_mat", "gen_n40"),
                 negative_det=name == "test_mat")


def test_gpu_step_lifecycle():
    check_lifecycle(None)


def test_gpu_pivot_update_rejects_bad_input():
    check_rejections(None)
