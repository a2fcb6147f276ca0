"""Bounds in the exact selections (slip_hip_ratio_test_bounded, slip_hip_bound_test and their fused forms on a handle) from the
HIP kernel SOURCE run lane by lane on the CPU (tests/emu), against Python fractions in the direct formulation: the reduction to
the unbounded ratio test, every width class of the form pass, signs, zeros and sides, unreduced ties, the launch geometry, the
bound test, handles on the two small goldens (one of them with a negative determinant) and every rejected input.  Small sizes
only: the emulator is slow."""
import os
import subprocess

import pytest

from bound_helpers import (check_bound_test, check_geometry, check_golden, check_negative_det, check_reduction, check_reduction_on_handle,
                           check_rejections, check_signs_and_sides, check_ties, check_width_classes)
from conftest import ROOT

EMU = os.path.join(ROOT, "tests", "emu", "libslip_emu.so")


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "libslip_emu.so"])
    return EMU


def test_emulated_bound_reduces_to_the_ratio_test(emu_lib):
    check_reduction(emu_lib)


def test_emulated_bound_reduces_to_the_ratio_test_on_a_handle(emu_lib):
    check_reduction_on_handle(emu_lib, "test_mat", waves=2)


def test_emulated_bound_width_classes(emu_lib):
    check_width_classes(emu_lib)


def test_emulated_bound_signs_zeros_sides(emu_lib):
    check_signs_and_sides(emu_lib)


def test_emulated_bound_unreduced_ties(emu_lib):
    check_ties(emu_lib)


def test_emulated_bound_geometry(emu_lib):
    check_geometry(emu_lib, (1, 63, 64, 65, 130))


def test_emulated_bound_test(emu_lib):
    check_bound_test(emu_lib)


@pytest.mark.parametrize("name", ["test_mat", "gen_n40"])
def test_emulated_bound_on_handles(emu_lib, name):
    # (gen_n40: one orientation, one combination; an emulated solve of four right-hand sides takes seconds)
    check_golden(emu_lib, name, light=name != "test_mat", transposes=(False, True) if name == "test_mat" else (False,), waves=2)


def test_emulated_bound_negative_determinant(emu_lib):
    check_negative_det(emu_lib, "test_mat", light=True, waves=2)


def test_emulated_bound_rejects_bad_input(emu_lib):
    check_rejections(emu_lib, "test_mat", waves=2)
