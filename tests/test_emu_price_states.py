"""Pricing with nonbasic states and reference weights (slip_hip_factor_price_states, slip_hip_price_select) from the HIP
kernel SOURCE run lane by lane on the CPU (tests/emu), against Python fractions on the true values: the launch geometry,
every degenerate outcome, a handle with a negative determinant, the existing calls it must agree with, every width class of
the squares, the grouping of both staging slabs, the lifecycle of a handle, every rejected input and the ABI.  Small sizes,
test_mat everywhere and one combination of (sense, key) per shape: the emulator is slow."""
import os
import subprocess

import pytest

from conftest import ROOT
from price_states_helpers import (check_abi, check_against_price, check_degenerate, check_geometry, check_groups, check_lifecycle,
                                  check_negative_det, check_rejections, check_width_classes)

EMU = os.path.join(ROOT, "tests", "emu", "libslip_emu.so")


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "libslip_emu.so"])
    return EMU


@pytest.mark.parametrize("ncols", [1, 63, 64, 65, 130])
def test_emulated_price_states_geometry(emu_lib, ncols):
    check_geometry(emu_lib, (ncols,), name="test_mat", light=True, waves=2)


def test_emulated_price_states_degenerate_outcomes(emu_lib):
    check_degenerate(emu_lib, "test_mat", waves=2)


def test_emulated_price_states_negative_determinant(emu_lib):
    assert check_negative_det(emu_lib, "test_mat", light=True, waves=2) < 0


def test_emulated_price_states_against_price(emu_lib):
    check_against_price(emu_lib, "test_mat", waves=2)


def test_emulated_price_states_width_classes(emu_lib):
    check_width_classes(emu_lib)


def test_emulated_price_states_groups(emu_lib, monkeypatch):
    check_groups(emu_lib, monkeypatch, "test_mat", waves=2)


def test_emulated_price_states_lifecycle(emu_lib):
    check_lifecycle(emu_lib, "test_mat", waves=2)


def test_emulated_price_states_rejects_bad_input(emu_lib):
    check_rejections(emu_lib, "test_mat", waves=2)


def test_price_states_abi(emu_lib):
    from slip_lu_amd import _lib
    lib = _lib.load(emu_lib)
    for name in check_abi():
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is not None
    assert len(lib.slip_hip_factor_price_states.argtypes) == 23 and len(lib.slip_hip_price_select.argtypes) == 26
