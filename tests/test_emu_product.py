"""The exact sparse products (slip_hip_factor_multiply, slip_hip_matrix_*) from the HIP kernel SOURCE run lane by lane on the
CPU (tests/emu), against Python integers: the synthetic corpus on both sides of every width class, handles on the two small
goldens, the lifecycle of a handle and every rejected input.  Small sizes only: the emulator is slow."""
import os
import subprocess

import pytest

from conftest import ROOT
from product_helpers import check_corpus, check_golden, check_groups, check_lifecycle, check_rejections, check_thin

EMU = os.path.join(ROOT, "tests", "emu", "libslip_emu.so")


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "libslip_emu.so"])
    return EMU


def test_emulated_product_corpus(emu_lib):
    check_corpus(emu_lib, wide_everywhere=False)


def test_emulated_product_in_groups(emu_lib, monkeypatch):
    check_groups(emu_lib, monkeypatch)


def test_emulated_product_thin_matrices(emu_lib):
    check_thin(emu_lib)


@pytest.mark.parametrize("name", ["test_mat", "gen_n40"])
def test_emulated_product_on_handles(emu_lib, name):
    check_golden(emu_lib, name, waves=2)


def test_emulated_product_lifecycle(emu_lib):
    check_lifecycle(emu_lib, waves=2)


def test_emulated_product_rejects_bad_input(emu_lib):
    check_rejections(emu_lib)
