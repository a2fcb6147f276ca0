"""The transposed solve (slip_hip_factor_solve_transpose: the view kernels and the substitutions on it) and its certificate
(slip_hip_factor_check_transpose) from the HIP kernel SOURCE run lane by lane on the CPU (tests/emu): the reference's
rationals of A^T x = b, the duality with the plain solve, the certificate's verdicts and rejections, the handle's
lifecycle, and helper workgroups on the view.  Small sizes only: the emulator is slow."""
import os
import subprocess

import pytest

from conftest import ROOT
from tsolve_helpers import (check_duality, check_duplicates, check_lifecycle, check_reference_tsolve, check_rejections,
                            check_verdicts)


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "libslip_emu.so"])
    return os.path.join(ROOT, "tests", "emu", "libslip_emu.so")


@pytest.fixture(scope="module")
def emu_farm_lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "libslip_emu_farm.so"])
    return os.path.join(ROOT, "tests", "emu", "libslip_emu_farm.so")


@pytest.mark.parametrize("name,nrhs,kw", [("tsolve_test_mat", 1, dict(waves=2, workers=1)),
                                          ("tsolve_gen_n40", 3, dict(waves=2, workers=2))])
def test_emulated_tsolve_matches_reference(emu_lib, name, nrhs, kw):
    check_reference_tsolve(emu_lib, name, nrhs=nrhs, **kw)


@pytest.mark.parametrize("name", ["test_mat", "gen_n40"])
def test_emulated_tsolve_duality(emu_lib, name):
    check_duality(emu_lib, name)


@pytest.mark.parametrize("name", ["test_mat", "gen_n40"])
def test_emulated_check_transpose_verdicts(emu_lib, name):
    check_verdicts(emu_lib, name)


def test_emulated_check_transpose_keeps_the_last_duplicate(emu_lib):
    check_duplicates(emu_lib)


def test_emulated_transpose_rejects_bad_input(emu_lib):
    check_rejections(emu_lib)


def test_emulated_tsolve_lifecycle(emu_lib):
    check_lifecycle(emu_lib, "solve_test_mat", waves=2, workers=2)


def test_emulated_tsolve_with_helpers(emu_farm_lib):
    """one right-hand side on five workgroups, in the build that opens every update queue of two or more items: the helpers
    run kinds 1 and 5 on the transposed view's parameters, same rationals"""
    assert check_reference_tsolve(emu_farm_lib, "tsolve_gen_n40", nrhs=1, waves=2, workers=5) > 0
