"""Solutions as reduced fractions (slip_reduce_kernel, slip_pack_kernel; slip_hip_solution_to_rational,
slip_hip_factor_solve_rational) from the HIP kernel SOURCE run lane by lane on the CPU (tests/emu), and the Python-integer model
of mpq_canonicalize the other tests compare with, against GMP's own answers (tests/golden/rational_corpus.json.gz)."""
import os
import subprocess

import pytest

from conftest import ROOT
from rational_helpers import (canonical, check_certificate, check_corpus, check_integer_solutions, check_lifecycle,
                              check_reference_solutions, check_reference_tsolutions, check_rejections, check_scale, corpus_mix,
                              load_corpus)


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "libslip_emu.so"])
    return os.path.join(ROOT, "tests", "emu", "libslip_emu.so")


def test_canonical_model_matches_gmp():
    """canonical == mpq_canonicalize on every corpus entry; the corpus holds the sizes and shapes the issue lists"""
    den, dpad, num, pad, want = load_corpus()
    assert 18 <= len(den) <= 30 and all(len(row) == len(num[0]) >= 20 for row in num)
    sizes = [abs(D).bit_length() for D in den]
    assert {1, 32, 33, 64, 65, 64 * 32, 64 * 32 + 1, 128 * 32, 128 * 32 + 1, 256 * 32, 257 * 32} <= set(sizes)
    assert 2 ** 32 in den and 2 ** 64 in den and any(8900 <= s <= 9100 for s in sizes)
    assert any(D > 2 ** 64 and D & (D - 1) == 0 for D in den)                                   # a power of two
    assert any(D % 2 ** 70 == 0 and D % 2 ** 71 and D >> 70 > 1 for D in den)                   # odd * 2^70
    assert sum(D < 0 for D in den) == 2 and dpad == [c % 2 for c in range(len(den))]
    for c, D in enumerate(den):
        a, bd, row = abs(D), abs(D).bit_length(), num[c]
        assert row[0] == 0 and D in row and -D in row and any(p == 1 for p in pad[c]) and any(p == 2 for p in pad[c])
        assert any(N.bit_length() >= 9 * bd for N in row) and any(N and abs(N).bit_length() <= bd // 10 + 1 for N in row)
        assert any(N and abs(N) > a and abs(N) % a == 0 for N in row)                           # an integer solution
        assert any(abs(n) == 1 for n, _ in want[c])                                             # N divides D
        assert any(0 < abs(N) < 2 ** 64 for N in row) and any(N < 0 for N in row)
        assert any(N > 0 and (N + 1) & N == 0 or (N ^ (N + 1)).bit_length() > bd // 2 for N in row)      # all-ones low digits
        gs = [a // d for _, d in want[c]]
        if bd > 300 and D & 1:
            assert any(31 <= g.bit_length() <= 33 for g in gs) and any(63 <= g.bit_length() <= 65 for g in gs)
            assert any(abs(g.bit_length() - bd // 2) <= bd // 20 for g in gs) and any(bd - 48 <= g.bit_length() <= bd - 32 for g in gs)
        if D % 2 == 0:
            assert any(g > 1 and g & (g - 1) == 0 for g in gs)                                  # a power of two alone
            assert any(g % 2 == 0 and g & (g - 1) for g in gs) or a & (a - 1) == 0              # 2^k * odd
        for t, N in enumerate(row):
            assert canonical(N, D) == want[c][t], (c, t)
    total, reduced, big_odd = corpus_mix(den, want, range(len(den)))
    assert 2 * reduced >= total and 4 * big_odd >= total


def test_canonical_semantics():
    assert canonical(0, -5) == (0, 1) and canonical(6, -4) == (-3, 2) and canonical(-6, -4) == (3, 2)
    assert canonical(2 ** 70, 2 ** 64) == (64, 1) and canonical(-7, 7) == (-1, 1)


def test_emulated_kernel_matches_gmp_corpus(emu_lib):
    """Left out: the denominators above 256 * 32 bits other than the one of 257 * 32 bits (the about 9000-bit one and the wide
    Fibonacci one; the emulator takes about a second per such entry).  What stays runs every path: the lane pass, the register
    classes with g = 1 and g > 1, and -- for the 257 * 32-bit denominator and the ten times longer numerators -- the memory class."""
    den = load_corpus()[0]
    keep = [c for c, D in enumerate(den) if abs(D).bit_length() <= 257 * 32]
    assert len(keep) == len(den) - 2 and any(abs(den[c]).bit_length() == 257 * 32 for c in keep)
    paths = check_corpus(emu_lib, keep)
    assert all(p > 0 for p in paths), paths


@pytest.mark.parametrize("name,kw", [("solve_test_mat", dict(waves=2, workers=1)), ("solve_gen_n40", dict(waves=2, workers=2))])
def test_emulated_solve_rational_matches_reference(emu_lib, name, kw):
    check_reference_solutions(emu_lib, name, nrhs=3, **kw)


@pytest.mark.parametrize("name,kw", [("tsolve_test_mat", dict(waves=2, workers=1)), ("tsolve_gen_n40", dict(waves=2, workers=2))])
def test_emulated_solve_rational_transposed_matches_reference(emu_lib, name, kw):
    check_reference_tsolutions(emu_lib, name, nrhs=3, **kw)


def test_emulated_integer_solutions_come_back_over_one(emu_lib):
    check_integer_solutions(emu_lib, "solve_gen_n40", waves=2, workers=2)


def test_emulated_scale(emu_lib):
    check_scale(emu_lib, "solve_test_mat", waves=2, workers=1)


def test_emulated_solve_rational_lifecycle(emu_lib):
    check_lifecycle(emu_lib, "solve_test_mat", waves=2, workers=2)


def test_emulated_solution_to_rational_rejects_bad_input(emu_lib):
    check_rejections(emu_lib)


def test_emulated_reduced_fractions_pass_the_exact_check(emu_lib):
    check_certificate(emu_lib, "solve_gen_n40", nrhs=3, waves=2, workers=2)
