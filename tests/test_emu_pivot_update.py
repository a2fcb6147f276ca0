"""The exact pivot update (slip_hip_pivot_update, slip_hip_factor_solve_update, slip_hip_factor_step) from the HIP kernel SOURCE
run lane by lane on the CPU (tests/emu), against Python integers and fractions: every width class of the form pass and every
kind of divisor, signs, zeros and the form without a division, inexact divisions of every path, placement and the launch
geometry, steps on the two small goldens with the end-to-end proof against the replaced basis and the dual form, the
lifecycle of a handle and every rejected input.  Small sizes only: the emulator is slow."""
import os
import subprocess

import pytest

from conftest import ROOT
from pivot_update_helpers import (check_geometry, check_golden, check_inexact, check_lane_carry, check_lifecycle, check_rejections,
                                  check_signs_and_zeros, check_width_classes)

EMU = os.path.join(ROOT, "tests", "emu", "libslip_emu.so")


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "libslip_emu.so"])
    return EMU


def test_emulated_pivot_update_width_classes(emu_lib):
    check_width_classes(emu_lib)


def test_emulated_pivot_update_signs_and_zeros(emu_lib):
    check_signs_and_zeros(emu_lib)


def test_emulated_pivot_update_lane_carry(emu_lib):
    check_lane_carry(emu_lib)


def test_emulated_pivot_update_inexact(emu_lib):
    check_inexact(emu_lib)


def test_emulated_pivot_update_geometry(emu_lib):
    check_geometry(emu_lib, (1, 63, 64, 65, 130))


@pytest.mark.parametrize("name", ["test_mat", "gen_n40"])
def test_emulated_step_on_handles(emu_lib, name):
    # (gen_n40: the proof alone; an emulated substitution of one right-hand side takes two seconds)
    if name == "test_mat":
        check_golden(emu_lib, name, light=True, proof=True, negative_det=True, waves=2)
    else:
        check_golden(emu_lib, name, light=True, transposes=(), proof=True, cross=False, waves=2)


def test_emulated_step_lifecycle(emu_lib):
    check_lifecycle(emu_lib, "test_mat", waves=2)


def test_emulated_pivot_update_rejects_bad_input(emu_lib):
    check_rejections(emu_lib, "test_mat", waves=2)
