"""Exact pricing (slip_hip_factor_price) from the HIP kernel SOURCE run lane by lane on the CPU (tests/emu), against Python
fractions and against the three-call route (solve_transpose + multiply + ratio_test) of the same build: the launch geometry,
the shapes of M, every width class of the product, handles on the two small goldens (one of them with a negative
determinant), the grouping of the staging slab, the lifecycle of a handle and every rejected input.  Small sizes, test_mat nearly
everywhere and one combination of (sense, key) per nside: the emulator is slow."""
import os
import subprocess

import pytest

from conftest import ROOT
from price_helpers import (check_geometry, check_golden, check_groups, check_lifecycle, check_rejections, check_shapes,
                           check_width_classes)

EMU = os.path.join(ROOT, "tests", "emu", "libslip_emu.so")


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "libslip_emu.so"])
    return EMU


@pytest.mark.parametrize("ncols", [1, 63, 64, 65, 130])
def test_emulated_price_geometry(emu_lib, ncols):
    check_geometry(emu_lib, (ncols,), name="test_mat", light=True, waves=2)


def test_emulated_price_shapes_of_m(emu_lib):
    check_shapes(emu_lib, "test_mat", combos=((1, False), (1, True)), waves=2)


def test_emulated_price_width_classes(emu_lib):
    check_width_classes(emu_lib, 6, "test_mat", combos=((-1, True),), sides=(1,), waves=2)


@pytest.mark.parametrize("name", ["test_mat", "gen_n40"])
def test_emulated_price_on_handles(emu_lib, name):
    # (gen_n40: the dual ratio test on the problem where all tie, alone; its emulated factorisation and solves take seconds each)
    if name == "test_mat":
        check_golden(emu_lib, name, combos=((1, False),), light=True, waves=2)
    else:
        check_golden(emu_lib, name, combos=((-1, True),), light=True, sides=(2,), waves=2)


def test_emulated_price_negative_determinant(emu_lib):
    assert check_golden(emu_lib, "test_mat", combos=((1, True), (-1, False)), light=True, negative=True, waves=2) < 0


def test_emulated_price_groups(emu_lib, monkeypatch):
    check_groups(emu_lib, monkeypatch, "test_mat", waves=2)


def test_emulated_price_lifecycle(emu_lib):
    check_lifecycle(emu_lib, "test_mat", waves=2)


def test_emulated_price_rejects_bad_input(emu_lib):
    check_rejections(emu_lib, "test_mat", waves=2)
