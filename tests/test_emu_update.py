"""The rewind to column K (slip_hip_factor_rewind: slip_rewind_kernel) and the replacement of a column of the resident A
(slip_hip_factor_replace_column: slip_splice_kernel, slip_offscan_kernel, slip_pack_kernel) from the HIP kernel SOURCE run
lane by lane on the CPU (tests/emu), against the CPU restatement on the matrix as it stands and the goldens.  Small sizes
only: the emulator is slow."""
import os
import subprocess

import pytest

from conftest import ROOT
from update_helpers import (check_certificate, check_q_tail, check_refusals, check_replace, check_replace_ahead,
                            check_rewind_equals_run, check_rewind_then_run, check_sequence, check_singular_repaired,
                            check_storage_bound)

KW = dict(waves=2, workers=2)


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "libslip_emu.so"])
    return os.path.join(ROOT, "tests", "emu", "libslip_emu.so")


@pytest.fixture(scope="module")
def emu_farm_lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "libslip_emu_farm.so"])
    return os.path.join(ROOT, "tests", "emu", "libslip_emu_farm.so")


# (gen_n40's eight-bit values cost the emulator 20 s per complete run, gen_n40_pm1's one-bit values one second: the rewinds
# run on the latter; gen_n40 is the device suite's)
@pytest.mark.parametrize("name,pivot,Ks,kw", [
    ("test_mat", 3, None, dict(waves=2, workers=1)), ("gen_n40_pm1", 3, range(0, 41, 5), KW), ("gen_n40_pm1", 0, (1, 17, 39), KW),
    ("gen_n40_pm1", 1, (2, 23), KW), ("gen_n40_pm1", 5, (7, 31), dict(waves=2, workers=1))])
def test_emulated_rewind_equals_run_to_K(emu_lib, name, pivot, Ks, kw):
    contested = check_rewind_equals_run(emu_lib, name, pivot, Ks, **kw)
    if pivot == 3:
        assert contested > 0            # positions the undo writes twice: the smallest column has to win there


@pytest.mark.parametrize("name,K,kw", [("test_mat", 4, dict(waves=2, workers=1)), ("gen_n40_pm1", 11, KW)])
def test_emulated_rewind_then_run_is_the_golden(emu_lib, name, K, kw):
    check_rewind_then_run(emu_lib, name, K, **kw)


def test_emulated_rewind_then_run_with_helpers(emu_farm_lib):
    check_rewind_then_run(emu_farm_lib, "gen_n40_pm1", 23, waves=2, workers=3)


@pytest.mark.parametrize("where,kind", [("first", "more"), ("middle", "fewer"), ("last", "single"), ("middle", "wide"),
                                        ("first", "dup"), ("last", "hizero"), ("middle", "single")])
def test_emulated_replace_column_against_oracle(emu_lib, where, kind):
    check_replace(emu_lib, "test_mat", where, kind, waves=2, workers=1)


@pytest.mark.parametrize("where,kind", [("middle", "more"), ("last", "wide")])
def test_emulated_replace_column_two_workers(emu_lib, where, kind):
    check_replace(emu_lib, "gen_n40_pm1", where, kind, **KW)


def test_emulated_replace_ahead_of_the_frontier(emu_lib):
    check_replace_ahead(emu_lib, "test_mat", waves=2, workers=2)


def test_emulated_replacement_sequence(emu_lib):
    check_sequence(emu_lib, "test_mat", steps=12, waves=2, workers=2)


def test_emulated_storage_bound(emu_lib):
    check_storage_bound(emu_lib, "test_mat", steps=64, waves=2, workers=1)


def test_emulated_singular_and_repaired(emu_lib):
    check_singular_repaired(emu_lib, "gen_n40_pm1", **KW)


def test_emulated_certificate_sees_the_new_matrix(emu_lib):
    check_certificate(emu_lib, "test_mat", waves=2, workers=1)


def test_emulated_q_tail(emu_lib):
    check_q_tail(emu_lib, "test_mat", waves=2, workers=2)


def test_emulated_refusals(emu_lib):
    check_refusals(emu_lib, "test_mat", waves=2, workers=1)
