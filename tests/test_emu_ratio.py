"""The exact ratio test (slip_hip_ratio_test, slip_hip_factor_ratio_test) from the HIP kernel SOURCE run lane by lane on the CPU
(tests/emu), against Python fractions: every width class of the exact comparison, unreduced ties, signs and zeros, the launch
geometry, integer vectors without denominators, handles on the two small goldens (one of them with a negative determinant),
the lifecycle of a handle and every rejected input.  Small sizes only: the emulator is slow."""
import os
import subprocess

import pytest

from conftest import ROOT
from ratio_helpers import (check_geometry, check_golden, check_lifecycle, check_negative_det, check_no_denominators, check_rejections,
                           check_signs_and_zeros, check_ties, check_width_classes)

EMU = os.path.join(ROOT, "tests", "emu", "libslip_emu.so")


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "libslip_emu.so"])
    return EMU


def test_emulated_ratio_width_classes(emu_lib):
    check_width_classes(emu_lib)


def test_emulated_ratio_unreduced_ties(emu_lib):
    check_ties(emu_lib)


def test_emulated_ratio_signs_and_zeros(emu_lib):
    check_signs_and_zeros(emu_lib)


def test_emulated_ratio_geometry(emu_lib):
    check_geometry(emu_lib, (1, 63, 64, 65, 130))


def test_emulated_ratio_without_denominators(emu_lib):
    check_no_denominators(emu_lib)


@pytest.mark.parametrize("name", ["test_mat", "gen_n40"])
def test_emulated_ratio_on_handles(emu_lib, name):
    # (gen_n40: one orientation, one combination; an emulated solve of four right-hand sides takes seconds)
    check_golden(emu_lib, name, light=name != "test_mat", transposes=(False, True) if name == "test_mat" else (False,), waves=2)


def test_emulated_ratio_negative_determinant(emu_lib):
    check_negative_det(emu_lib, "test_mat", light=True, waves=2)


def test_emulated_ratio_lifecycle(emu_lib):
    check_lifecycle(emu_lib, light=True, waves=2)


def test_emulated_ratio_rejects_bad_input(emu_lib):
    check_rejections(emu_lib, "test_mat", waves=2)
