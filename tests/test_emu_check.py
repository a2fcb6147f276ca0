"""The exact solution check (slip_hip_factor_check, slip_hip_check_solution) from the HIP kernel SOURCE run lane by lane
on the CPU (tests/emu): verdicts against exact Python-integer residuals, against the reference's own rational solutions,
on the register and the memory paths, and every rejected input.  Small sizes only: the emulator is slow."""
import os
import subprocess

import pytest

from check_helpers import (check_clean, check_duplicates, check_error_paths, check_perturbations, check_reference_rationals,
                           check_wide, factor_and_solve, rhs_pair)
from conftest import ROOT, load_case

EMU = os.path.join(ROOT, "tests", "emu", "libslip_emu.so")


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "libslip_emu.so"])
    return EMU


@pytest.mark.parametrize("name", ["test_mat", "gen_n40"])
def test_emulated_check_of_solves(emu_lib, name):
    """one factorisation and one 3-rhs solve per case (the emulated factorisation is the slow part): clean, then perturbed"""
    _, fix = load_case(name)
    n, Ap, Ai, Alen, Alimbs, q = len(fix["q"]), fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"]
    bs = rhs_pair(n)
    f, x, det = factor_and_solve(emu_lib, n, Ap, Ai, Alen, Alimbs, q, bs)
    try:
        check_clean(f, n, x, bs)
        check_perturbations(f, n, Ap, Ai, Alen, Alimbs, q, x, det, bs)
    finally:
        f.close()


@pytest.mark.parametrize("name", ["solve_test_mat", "solve_gen_n40", "solve_10teams"])
def test_emulated_check_of_reference_rationals(emu_lib, name):
    check_reference_rationals(emu_lib, name)


@pytest.mark.parametrize("ylimbs", [150, 400])
def test_emulated_check_wide_path(emu_lib, ylimbs):
    check_wide(emu_lib, 30, ylimbs, 3, ylimbs)


def test_emulated_check_keeps_the_last_duplicate(emu_lib):
    check_duplicates(emu_lib)


def test_emulated_check_rejects_bad_input(emu_lib):
    check_error_paths(emu_lib)
