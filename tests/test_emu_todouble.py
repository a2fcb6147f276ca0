"""Solutions as doubles (slip_todouble_kernel, slip_scale_kernel; slip_hip_solution_to_double, slip_hip_factor_solve_double)
from the HIP kernel SOURCE run lane by lane on the CPU (tests/emu), and the Python-integer model of mpq_get_d the other tests
compare with, against GMP's own answers (tests/golden/todouble_corpus.json.gz).  Small sizes only: the emulator is slow."""
import os
import subprocess

import pytest

from conftest import ROOT
from todouble_helpers import (bits, check_corpus, check_integer_solutions, check_lifecycle, check_reference_solutions,
                              check_reference_tsolutions, check_rejections, check_scale, is_boundary, load_corpus, trunc_double)


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "libslip_emu.so"])
    return os.path.join(ROOT, "tests", "emu", "libslip_emu.so")


def test_trunc_double_model_matches_gmp():
    """trunc_double == mpq_get_d on every corpus entry, bit for bit; the corpus holds what the issue lists"""
    den, num, pad, want = load_corpus()
    assert 20 <= len(den) <= 30 and all(20 <= len(row) <= 30 for row in num)
    sizes = sorted(abs(D).bit_length() for D in den)
    assert sizes[0] == 1 and {53, 64, 65, 128, 1000} <= set(sizes) and sum(s > 8192 for s in sizes) >= 2
    assert sum(2900 <= s <= 3100 for s in sizes) >= 2 and any(D < 0 for D in den) and any(p for row in pad for p in row)
    for c, D in enumerate(den):
        for t, N in enumerate(num[c]):
            assert bits(trunc_double(N, D)) == want[c][t], (c, t)
    total = sum(len(row) for row in num)
    assert 3 * sum(is_boundary(N, den[c]) for c in range(len(den)) for N in num[c]) >= total


def test_trunc_double_semantics():
    """the cases the issue spells out"""
    assert trunc_double(2 ** 1024 - 1, 1).hex() == "0x1.fffffffffffffp+1023"
    assert trunc_double(-3, 2 ** 1075).hex() == "-0x0.0000000000001p-1022"
    assert bits(trunc_double(-1, 2 ** 1075)) == bits(0.0) and bits(trunc_double(0, -5)) == bits(0.0)
    assert trunc_double(2 ** 1024, 1) == float("inf") and trunc_double(2 ** 1024, -1) == float("-inf")
    assert trunc_double(2 ** 53 + 1, 1) == 2.0 ** 53 and trunc_double(-(2 ** 54 - 1), 1) == -(2.0 ** 54 - 2)


def test_emulated_kernel_matches_gmp_corpus(emu_lib):
    """the whole corpus in one call, the operands above 8192 bits included (well under a second in the emulator: no subset)"""
    assert check_corpus(emu_lib) >= 25 * 24


@pytest.mark.parametrize("name,kw", [("solve_test_mat", dict(waves=2, workers=1)), ("solve_gen_n40", dict(waves=2, workers=2))])
def test_emulated_solve_double_matches_reference(emu_lib, name, kw):
    check_reference_solutions(emu_lib, name, nrhs=3, **kw)


@pytest.mark.parametrize("name,kw", [("tsolve_test_mat", dict(waves=2, workers=1)), ("tsolve_gen_n40", dict(waves=2, workers=2))])
def test_emulated_solve_double_transposed_matches_reference(emu_lib, name, kw):
    check_reference_tsolutions(emu_lib, name, nrhs=3, **kw)


def test_emulated_integer_solutions_come_back_exactly(emu_lib):
    assert check_integer_solutions(emu_lib, "solve_gen_n40", waves=2, workers=2) > 0      # they do take the wave pass


def test_emulated_scale(emu_lib):
    check_scale(emu_lib, "solve_test_mat", waves=2, workers=1)


def test_emulated_solve_double_lifecycle(emu_lib):
    check_lifecycle(emu_lib, "solve_test_mat", waves=2, workers=2)


def test_emulated_solution_to_double_rejects_bad_input(emu_lib):
    check_rejections(emu_lib)
