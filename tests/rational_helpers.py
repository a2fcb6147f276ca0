"""Shared by tests/test_emu_rational.py (the emulator build) and tests/test_gpu_rational.py (the product on the device): exact
solutions as reduced fractions (slip_hip_solution_to_rational, slip_hip_factor_solve_rational) against canonical, a model in
Python integers of what GMP's mpq_canonicalize leaves, and against GMP's own answers recorded in
tests/golden/rational_corpus.json.gz.  Every comparison is of signs and limbs.  lib_path None is the product library."""
import gzip
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import oracle_lib
import slabfile
from check_helpers import slab
from conftest import GOLDEN, load_case, solve_inputs
from todouble_helpers import SCALES, SOLVE_CASES, TSOLVE_CASES, handle, integer_rhs, padded_slab, rhs_pattern


def canonical(N, D):
    """(num, den) of N / D (D != 0) in lowest terms with den > 0, the sign on num and 0 as 0 / 1: GMP's canonical form"""
    if D == 0:
        raise ZeroDivisionError("canonical: zero denominator")
    g = math.gcd(N, D)
    s = -1 if D < 0 else 1
    return s * N // g, s * D // g


def load_corpus():
    """(denominators, their high zero limbs, numerators per denominator, high zero limbs per numerator, GMP's (num, den))"""
    doc = json.loads(gzip.open(os.path.join(GOLDEN, "rational_corpus.json.gz")).read())
    den = [int(v, 16) for v in doc["den"]]
    num = [[int(v, 16) for v in row] for row in doc["num"]]
    want = [[(int(a, 16), int(b, 16)) for a, b in zip(ra, rb)] for ra, rb in zip(doc["cnum"], doc["cden"])]
    return den, doc["dpad"], num, doc["pad"], want


def corpus_mix(den, want, keep):
    """(entries, those with g > 1, those with an odd g above 64 bits) of the kept denominators, from GMP's answers alone"""
    gs = [abs(den[c]) // d for c in keep for _, d in want[c]]
    return len(gs), sum(g > 1 for g in gs), sum(g & 1 and g.bit_length() > 64 for g in gs)


def fractions_of(result, count):
    """(numlen, numlimbs, denlen, denlimbs) -> [(num, den)], after checking the layout: `count` entries, the slabs compact (the
    counts add up to the limbs returned) and normalised (no high zero limb), every denominator at least one limb and positive"""
    numlen, numlimbs, denlen, denlimbs = result
    assert numlen.size == count and denlen.size == count
    assert int(np.abs(numlen.astype(np.int64)).sum()) == numlimbs.size and int(denlen.astype(np.int64).sum()) == denlimbs.size
    assert (denlen >= 1).all()
    for lens, limbs in ((numlen, numlimbs), (denlen, denlimbs)):
        ends = np.cumsum(np.abs(lens.astype(np.int64)))
        tops = limbs[ends[lens != 0] - 1]
        assert (tops != 0).all(), "a high zero limb"
    return list(zip(oracle_lib.bigints(numlen, numlimbs), oracle_lib.bigints(denlen, denlimbs)))


def assert_same_fractions(got, want, what):
    assert got == want, (what, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:3])


def check_corpus(lib_path, keep=None):
    """the corpus (or its denominators `keep`) in ONE call, n = numerators per denominator, nrhs = denominators: every
    (num, den) equals GMP's, signs and limbs.  Of what is run at least half has g > 1 and a quarter an odd g above 64 bits.
    Returns the entries settled by each of the kernel's four paths."""
    import slip_lu_amd as sl
    den, dpad, num, pad, want = load_corpus()
    keep = list(range(len(den))) if keep is None else list(keep)
    n = len(num[0])
    total, reduced, big_odd = corpus_mix(den, want, keep)
    assert total == n * len(keep) and 2 * reduced >= total and 4 * big_odd >= total, (total, reduced, big_odd)
    xlen, xlimbs = padded_slab([N for c in keep for N in num[c]], [p for c in keep for p in pad[c]])
    dlen, dlimbs = padded_slab([den[c] for c in keep], [dpad[c] for c in keep])
    got = fractions_of(sl.solution_to_rational(n, xlen, xlimbs, dlen, dlimbs, nrhs=len(keep), lib_path=lib_path), total)
    paths = sl.solution_to_rational_paths(lib_path=lib_path)
    assert sum(paths) == total, paths
    assert all(d > 0 for _, d in got)
    assert_same_fractions(got, [w for c in keep for w in want[c]], "corpus")
    return paths


def placed(vals, q):
    """values by pivot position -> by original column (SLIP_permute_x)"""
    out = [None] * len(vals)
    for p, v in enumerate(vals):
        out[int(q[p])] = v
    return out


def check_reference_solutions(lib_path, name, nrhs=3, **kw):
    """solve_rational of solve_rhs(n) == the reference's own canonical xnum / xden (tests/golden/solve_*), placed at q[p]; the
    further right-hand sides == canonical() of the same handle's `solve` numerators over det.  Returns the path counts."""
    n, Ap, Ai, Alen, Alimbs, q, fix = solve_inputs(SOLVE_CASES[name])
    num = oracle_lib.bigints(fix["xnumlen"], fix["xnumlimbs"])
    den = oracle_lib.bigints(fix["xdenlen"], fix["xdenlimbs"])
    bs = rhs_pattern(oracle_lib.solve_rhs(n), nrhs)
    blen, blimbs = slab([v for b in bs for v in b])
    f, det = handle(lib_path, n, Ap, Ai, Alen, Alimbs, q, **kw)
    try:
        got = fractions_of(f.solve_rational(blen, blimbs, nrhs=nrhs), n * nrhs)
        assert f.to_rational_ms() >= 0
        paths = f.to_rational_paths()
        x = oracle_lib.bigints(*f.solve(blen, blimbs, nrhs=nrhs))
    finally:
        f.close()
    assert sum(paths) == n * nrhs
    assert_same_fractions(got[:n], placed(list(zip(num, den)), q), name)
    for c in range(nrhs):
        assert_same_fractions(got[c * n:(c + 1) * n], placed([canonical(x[c * n + p], det) for p in range(n)], q), (name, c))
    return paths


def check_reference_tsolutions(lib_path, name, nrhs=3, **kw):
    """the same for the transposed solve: b[k] = solve_rhs(n)[q[k]] gives the reference's solution of A^T x = solve_rhs(n)
    (tests/golden/tsolve_*, mapped by its own q_T), by original row id"""
    case = TSOLVE_CASES[name]
    n, Ap, Ai, Alen, Alimbs, q, _ = solve_inputs(SOLVE_CASES[case["source"]])
    fix = slabfile.load(os.path.join(GOLDEN, name + ".slab.gz"))
    num = oracle_lib.bigints(fix["xnumlen"], fix["xnumlimbs"])
    den = oracle_lib.bigints(fix["xdenlen"], fix["xdenlimbs"])
    b0 = oracle_lib.solve_rhs(n)
    bs = rhs_pattern(np.array([b0[int(q[k])] for k in range(n)]), nrhs)
    blen, blimbs = slab([v for b in bs for v in b])
    f, det = handle(lib_path, n, Ap, Ai, Alen, Alimbs, q, **kw)
    try:
        got = fractions_of(f.solve_rational(blen, blimbs, nrhs=nrhs, transpose=True), n * nrhs)
        x = oracle_lib.bigints(*f.solve_transpose(blen, blimbs, nrhs=nrhs))
    finally:
        f.close()
    assert_same_fractions(got[:n], placed(list(zip(num, den)), fix["q"]), name)
    for c in range(nrhs):
        assert_same_fractions(got[c * n:(c + 1) * n], [canonical(x[c * n + i], det) for i in range(n)], (name, c))


def check_integer_solutions(lib_path, name, **kw):
    """b = A(:,q) x0 with integer x0 (a third of it zero, some of several limbs): every fraction is x0 / 1, at q[p]"""
    n, Ap, Ai, Alen, Alimbs, q, _ = solve_inputs(SOLVE_CASES[name])
    x0 = [0 if p % 3 == 0 else ((p * 7919) % 41) - 20 for p in range(n)]
    x0[1], x0[2] = 2 ** 130 - 1, -(2 ** 64 + 1)
    blen, blimbs = slab(integer_rhs(n, Ap, Ai, Alen, Alimbs, q, x0))
    f, det = handle(lib_path, n, Ap, Ai, Alen, Alimbs, q, **kw)
    try:
        got = fractions_of(f.solve_rational(blen, blimbs), n)
    finally:
        f.close()
    assert_same_fractions(got, placed([(v, 1) for v in x0], q), name)


def check_scale(lib_path, name, **kw):
    """scale = snum / sden applied once, exactly: canonical(xnum * snum, det * sden), for the plain solve (as a pair and as a
    Fraction) and the transposed one; a zero scale part is SLIP_HIP_INCORRECT_INPUT"""
    import slip_lu_amd as sl
    n, Ap, Ai, Alen, Alimbs, q, _ = solve_inputs(SOLVE_CASES[name])
    bs = rhs_pattern(oracle_lib.solve_rhs(n), 2)
    blen, blimbs = slab([v for b in bs for v in b])
    f, det = handle(lib_path, n, Ap, Ai, Alen, Alimbs, q, **kw)
    try:
        x = oracle_lib.bigints(*f.solve(blen, blimbs, nrhs=2))
        xt = oracle_lib.bigints(*f.solve_transpose(blen, blimbs, nrhs=2))
        for sn, sd in SCALES:
            got = fractions_of(f.solve_rational(blen, blimbs, nrhs=2, scale=(sn, sd)), 2 * n)
            for c in range(2):
                want = placed([canonical(x[c * n + p] * sn, det * sd) for p in range(n)], q)
                assert_same_fractions(got[c * n:(c + 1) * n], want, (name, sn, sd, c))
            got = fractions_of(f.solve_rational(blen, blimbs, nrhs=2, transpose=True, scale=(sn, sd)), 2 * n)
            assert_same_fractions(got, [canonical(v * sn, det * sd) for v in xt], (name, "T", sn, sd))
        got = fractions_of(f.solve_rational(blen, blimbs, nrhs=2, scale=Fraction(3, 7)), 2 * n)
        assert_same_fractions(got, fractions_of(f.solve_rational(blen, blimbs, nrhs=2, scale=(3, 7)), 2 * n), "Fraction")
        for bad in ((0, 1), (1, 0), (0, 0)):
            with pytest.raises(sl.SlipError) as e:
                f.solve_rational(blen, blimbs, nrhs=2, scale=bad)
            assert e.value.code == -3
    finally:
        f.close()


def check_lifecycle(lib_path, name="solve_test_mat", **kw):
    """refused before the factorisation is complete, for nrhs < 1, and -- plain only -- on a handle around given factors (it holds
    no q; the transposed call works there); the same fractions after reset + run and after a GROW_X forced by a right-hand side
    of several limbs; `solve` and `solve_double` still return what they did"""
    import slip_lu_amd as sl
    n, Ap, Ai, Alen, Alimbs, q, _ = solve_inputs(SOLVE_CASES[name])
    b = [int(v) for v in oracle_lib.solve_rhs(n)]
    wide = [v * (2 ** 2000 + 12345) if k % 4 else 0 for k, v in enumerate(b)]      # 32 limbs
    blen, blimbs = slab(b)
    wlen, wlimbs = slab(wide)
    f = sl.Factorization(n, Ap, Ai, Alen, Alimbs, q, lib_path=lib_path, **kw)
    try:
        f.run(n // 2)
        for tr in (False, True):
            with pytest.raises(sl.SlipError) as e:
                f.solve_rational(blen, blimbs, transpose=tr)
            assert e.value.code == -3
        f.run(0)
        with pytest.raises(sl.SlipError) as e:
            f.solve_rational(blen[:0], blimbs, nrhs=0)
        assert e.value.code == -3
        det = oracle_lib.bigints(*f.pivots())[-1]
        x0 = f.solve(blen, blimbs)
        d0 = f.solve_double(blen, blimbs)
        r0 = fractions_of(f.solve_rational(blen, blimbs), n)
        t0 = fractions_of(f.solve_rational(blen, blimbs, transpose=True), n)
        assert_same_fractions(r0, placed([canonical(v, det) for v in oracle_lib.bigints(*x0)], q), "first")
        xcap = f.info()["xcap_digits"]
        rw = fractions_of(f.solve_rational(wlen, wlimbs), n)       # x needs 63 more digits than it did for b: the stride grows
        assert f.info()["xcap_digits"] > xcap
        xw = oracle_lib.bigints(*f.solve(wlen, wlimbs))
        assert_same_fractions(rw, placed([canonical(v, det) for v in xw], q), "wide right-hand side")
        assert_same_fractions(fractions_of(f.solve_rational(blen, blimbs), n), r0, "after the growth")
        x1 = f.solve(blen, blimbs)
        assert np.array_equal(x0[0], x1[0]) and np.array_equal(x0[1], x1[1])
        assert f.solve_double(blen, blimbs).tobytes() == d0.tobytes()
        fac = f.download()
        f.reset()
        with pytest.raises(sl.SlipError):
            f.solve_rational(blen, blimbs)
        f.run(0)
        assert_same_fractions(fractions_of(f.solve_rational(blen, blimbs), n), r0, "after reset + run")
        assert_same_fractions(fractions_of(f.solve_rational(blen, blimbs, transpose=True), n), t0, "transposed, after reset + run")
    finally:
        f.close()
    g = sl.Factorization.from_factors(fac, lib_path=lib_path, **{k: v for k, v in kw.items() if k in ("waves", "workers")})
    try:
        with pytest.raises(sl.SlipError) as e:
            g.solve_rational(blen, blimbs)
        assert e.value.code == -3
        assert_same_fractions(fractions_of(g.solve_rational(blen, blimbs, transpose=True), n), t0, "from factors, transposed")
    finally:
        g.close()


def check_rejections(lib_path):
    """slip_hip_solution_to_rational: nrhs < 1, a zero denominator (also as one limb that is zero), capacities one limb short"""
    import ctypes as C
    import slip_lu_amd as sl
    from slip_lu_amd import _lib
    lib = _lib.load(lib_path)
    xlen, xlimbs = slab([6, -7, 2 ** 64, 0])
    dlen, dlimbs = slab([-4])
    got = fractions_of(sl.solution_to_rational(4, xlen, xlimbs, dlen, dlimbs, lib_path=lib_path), 4)
    assert got == [(-3, 2), (7, 4), (-2 ** 62, 1), (0, 1)]
    out = [C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_void_p(), C.c_int64()]
    refs = [C.byref(o) for o in out]

    def call(n, nrhs, xcap, dl, dlim, dcap):
        rc = lib.slip_hip_solution_to_rational(n, nrhs, xlen.ctypes.data, xlimbs.ctypes.data, xcap, dl.ctypes.data, dlim.ctypes.data,
                                               dcap, *refs, None)
        assert rc == 0 or all(not o.value for o in out)          # nothing is handed out with an error
        return rc
    assert call(4, 0, xlimbs.size, dlen, dlimbs, 1) == -3
    assert call(4, 1, xlimbs.size - 1, dlen, dlimbs, 1) == -3
    assert call(4, 1, xlimbs.size, dlen, dlimbs, 0) == -3
    assert call(4, 1, xlimbs.size, np.zeros(1, np.int32), dlimbs, 1) == -3
    assert call(4, 1, xlimbs.size, np.array([1], np.int32), np.zeros(1, np.uint64), 1) == -3      # one limb that is zero


def check_wide_handle(lib_path, name):
    """a complete factorisation whose determinant exceeds 256 digits (the kernel's memory class): solve_rational ==
    canonical() of the same handle's `solve` numerators over det, entry by entry; an integer solution comes back as x0 / 1"""
    entry, fix = load_case(name)
    n, q = len(fix["q"]), fix["q"]
    f, det = handle(lib_path, n, fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], q, pivot=entry["pivot"], tol=entry["tol"])
    try:
        assert det.bit_length() > 256 * 32
        b = [int(v) for v in oracle_lib.solve_rhs(n)]
        x0 = [((p * 31) % 7) - 3 for p in range(n)]
        bi = integer_rhs(n, fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], q, x0)
        blen, blimbs = slab(b + bi)
        got = fractions_of(f.solve_rational(blen, blimbs, nrhs=2), 2 * n)
        paths = f.to_rational_paths()
        x = oracle_lib.bigints(*f.solve(blen, blimbs, nrhs=2))
    finally:
        f.close()
    for c in range(2):
        assert_same_fractions(got[c * n:(c + 1) * n], placed([canonical(x[c * n + p], det) for p in range(n)], q), (name, c))
    assert_same_fractions(got[n:], placed([(v, 1) for v in x0], q), (name, "integers"))
    assert paths[3] > 0 and sum(paths) == 2 * n, paths


def check_certificate(lib_path, name="solve_gen_n40", nrhs=3, **kw):
    """the returned fractions of each right-hand side brought to their lcm in Python pass check_solution: the reduced output
    composes with the exact certificate A x = d b"""
    import slip_lu_amd as sl
    n, Ap, Ai, Alen, Alimbs, q, _ = solve_inputs(SOLVE_CASES[name])
    bs = rhs_pattern(oracle_lib.solve_rhs(n), nrhs)
    blen, blimbs = slab([v for b in bs for v in b])
    f, det = handle(lib_path, n, Ap, Ai, Alen, Alimbs, q, **kw)
    try:
        got = fractions_of(f.solve_rational(blen, blimbs, nrhs=nrhs), n * nrhs)
    finally:
        f.close()
    xs, ds = [], []
    for c in range(nrhs):
        row = got[c * n:(c + 1) * n]
        d = math.lcm(*[dd for _, dd in row])
        xs += [nn * (d // dd) for nn, dd in row]
        ds.append(d)
    xlen, xlimbs = slab(xs)
    dlen, dlimbs = slab(ds)
    ok, first, bad = sl.check_solution(n, Ap, Ai, Alen, Alimbs, blen, blimbs, xlen, xlimbs, dlen, dlimbs, nrhs=nrhs, lib_path=lib_path)
    assert ok and list(first) == [-1] * nrhs and list(bad) == [0] * nrhs
