"""The bounded exact simplex step (slip_hip_step_bounded, slip_hip_factor_step_bounded) from the HIP kernel SOURCE run lane by
lane on the CPU (tests/emu), against Python integers and fractions in the direct formulation on the true values: the three
moves with ties, both sides and x outside its bounds, the width classes of slip_bstep_kernel, the reduction to
Factorization.step, the end-to-end proof of a pivot and of a flip, inexact divisions, more than one staging group, the
lifecycle of a handle and every refused input.  Small sizes only: the emulator is slow."""
import os
import subprocess

import pytest

from conftest import ROOT
from step_bounded_helpers import (check_groups, check_inexact, check_lifecycle, check_moves, check_proof, check_reduction,
                                  check_rejections, check_width_classes)

EMU = os.path.join(ROOT, "tests", "emu", "libslip_emu.so")


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "libslip_emu.so"])
    return EMU


def test_emulated_step_bounded_moves(emu_lib):
    check_moves(emu_lib, (1, 63, 64, 65))


def test_emulated_step_bounded_width_classes(emu_lib):
    check_width_classes(emu_lib, sizes=(4, 64), memory=260)


def test_emulated_step_bounded_reduction(emu_lib):
    check_reduction(emu_lib, "test_mat", waves=2)


def test_emulated_step_bounded_proof(emu_lib):
    check_proof(emu_lib, "test_mat", negative_det=True, waves=2)


def test_emulated_step_bounded_inexact(emu_lib):
    check_inexact(emu_lib)


def test_emulated_step_bounded_groups(emu_lib):
    check_groups(emu_lib, n=65)


def test_emulated_step_bounded_lifecycle(emu_lib):
    check_lifecycle(emu_lib, "test_mat", waves=2)


def test_emulated_step_bounded_rejects_bad_input(emu_lib):
    check_rejections(emu_lib, "test_mat", waves=2)
