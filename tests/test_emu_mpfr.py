"""Solutions as multi-precision floats (slip_mpfr_kernel, slip_scale_kernel; slip_hip_solution_to_mpfr,
slip_hip_factor_solve_mpfr) from the HIP kernel SOURCE run lane by lane on the CPU (tests/emu), and the Python-integer model of
mpfr_set_q the other tests compare with, against MPFR's own answers (tests/golden/mpfr_corpus.json.gz).  Small sizes only: the
emulator is slow."""
import os
import subprocess

import pytest

from conftest import ROOT
from mpfr_helpers import (MODES, RNDA, RNDZ, check_corpus, check_integer_solutions, check_lifecycle, check_reference_solutions,
                          check_reference_tsolutions, check_rejections, check_scale, load_corpus, round_mpfr)


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "libslip_emu.so"])
    return os.path.join(ROOT, "tests", "emu", "libslip_emu.so")


def test_round_mpfr_model_matches_mpfr():
    """round_mpfr == mpfr_set_q on every corpus entry under every mode, ternary included; the corpus holds what the issue lists"""
    co = load_corpus()
    den, precs = co["den"], co["prec"]
    sizes = sorted(abs(D).bit_length() for D in den)
    assert 11 <= len(den) <= 13 and sizes[0] == 1 and {2, 64, 65, 1000, 1001} <= set(sizes) and any(D < 0 for D in den)
    assert 2 ** 63 in den and 2 ** 1000 in den and any(2900 <= s <= 3100 for s in sizes) and sum(s > 8192 for s in sizes) >= 2
    assert precs == [2, 24, 53, 64, 65, 128, 200, 1000, 8300] and all(any(pad) for pad in co["pad"][:-1])
    assert len(co["prec_den"][precs.index(8300)]) == 2 and all(len(k) == len(den) for k in co["prec_den"][:-1])
    total = decisive = carries = 0
    ties = set()
    for c, D in enumerate(den):
        for pi, p in enumerate(precs):
            for t, N in enumerate(co["rows"][c][pi]):
                want = co["res"][c][pi][t]
                for rnd in MODES:
                    assert round_mpfr(N, D, p, rnd) == tuple(want[rnd]), (c, p, t, rnd)
                total += 1
                decisive += want[RNDZ] != want[RNDA]
                carries += want[RNDZ][1] != want[RNDA][1]                          # the upward modes carry into the exponent
                _, e, m, _ = want[RNDZ]                                            # the truncated mantissa
                if N and (2 * abs(N)) << max(p - e, 0) == ((2 * m + 1) * abs(D)) << max(e - p, 0):
                    ties.add(m & 1)                                                # an exact tie: |N / D| = (m + 1/2) * 2^(e - p)
    assert ties == {0, 1} and carries >= len(den) and 3 * decisive >= total, (ties, carries, decisive, total)
    assert any(abs(D).bit_length() > 8192 and co["rows"][c][precs.index(8300)] for c, D in enumerate(den))
    big = [abs(N).bit_length() - abs(D).bit_length() for c, D in enumerate(den) for N in co["rows"][c][0] if N]
    assert min(big) < -2000 and max(big) > 2000


def test_round_mpfr_semantics():
    """the cases the issue spells out"""
    assert round_mpfr(7, 2, 2, 0) == (1, 3, 2, 1)                                  # 3.5 -> 4 = 0.10b * 2^3
    assert round_mpfr(2 ** 64 - 1, 1, 10, 0) == (1, 65, 2 ** 9, 1)
    assert round_mpfr(0, -5, 53, 3) == (0, 0, 0, 0)
    assert round_mpfr(5, 2, 2, 0) == (1, 2, 2, -1) and round_mpfr(7, 2, 3, 0) == (1, 2, 7, 0)     # ties to even; exact
    assert round_mpfr(-1, 3, 4, 2)[3] == 1 and round_mpfr(-1, 3, 4, 3)[3] == -1 and round_mpfr(-1, 3, 4, 4)[3] == -1
    for bad in ((1, 0), (65537, 0), (53, 5), (53, -1)):
        with pytest.raises(ValueError):
            round_mpfr(1, 3, *bad)


@pytest.mark.parametrize("prec", [2, 24, 53, 64, 65, 128, 200, 1000, 8300])
def test_emulated_kernel_matches_mpfr_corpus(emu_lib, prec):
    """the whole corpus, one call per (precision, mode), the operands above 8192 bits and the precision above 256 digits
    included; every path is taken: the lane pass within 64 bits (up to 64 bits of precision), the long division with a
    denominator of at most 256 digits and with a wider one, the zeros"""
    total, paths = check_corpus(emu_lib, precs=[prec])
    assert total == (5 * 28 * 12 if prec != 8300 else 5 * 6 * 2) and sum(paths) == total
    assert (paths[0] > 0) == (prec <= 64) and (paths[1] > 0) == (prec != 8300) and paths[2] > 0 and paths[3] > 0, paths


@pytest.mark.parametrize("name,kw", [("solve_test_mat", dict(waves=2, workers=1)), ("solve_gen_n40", dict(waves=2, workers=2))])
def test_emulated_solve_mpfr_matches_reference(emu_lib, name, kw):
    check_reference_solutions(emu_lib, name, nrhs=3, **kw)


@pytest.mark.parametrize("name,kw", [("tsolve_test_mat", dict(waves=2, workers=1)), ("tsolve_gen_n40", dict(waves=2, workers=2))])
def test_emulated_solve_mpfr_transposed_matches_reference(emu_lib, name, kw):
    check_reference_tsolutions(emu_lib, name, nrhs=3, **kw)


def test_emulated_integer_solutions_come_back_exactly(emu_lib):
    paths = check_integer_solutions(emu_lib, "solve_gen_n40", waves=2, workers=2)
    assert paths[1] > 0                                                            # the nonzero ones are long divisions


def test_emulated_scale(emu_lib):
    check_scale(emu_lib, "solve_test_mat", waves=2, workers=1)


def test_emulated_solve_mpfr_lifecycle(emu_lib):
    check_lifecycle(emu_lib, "solve_test_mat", waves=2, workers=2)


def test_emulated_mpfr_rejects_bad_input(emu_lib):
    check_rejections(emu_lib, "solve_test_mat", waves=2, workers=1)
