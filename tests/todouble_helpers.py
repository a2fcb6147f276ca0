"""Shared by tests/test_emu_todouble.py (the emulator build) and tests/test_gpu_todouble.py (the product on the device): the
conversion of exact solutions to doubles (slip_hip_solution_to_double, slip_hip_factor_solve_double) against trunc_double, a
model in Python integers of what GMP's mpq_get_d returns, and against GMP's own answers recorded in
tests/golden/todouble_corpus.json.gz.  Every comparison is of the 8 bytes, so +0.0 and -0.0 differ.  lib_path None is the
product library."""
import gzip
import json
import math
import os
import struct
from fractions import Fraction

import numpy as np
import pytest

import oracle_lib
import slabfile
from check_helpers import columns, slab
from conftest import GOLDEN, load_case, solve_inputs

SOLVE_CASES = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "solve_index.json")))}
TSOLVE_CASES = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "tsolve_index.json")))}


def trunc_double(num, den):
    """num / den (den != 0) truncated toward zero onto the double grid, as mpq_get_d does: 53 significant bits in the normal
    range, a multiple of 2^-1074 below 2^-1022, +0.0 when nothing is left (the sign is dropped), +-inf from 2^1024 on"""
    if den == 0:
        raise ZeroDivisionError("trunc_double: zero denominator")
    neg = (num < 0) != (den < 0)
    n, d = abs(num), abs(den)
    if n == 0:
        return 0.0
    e = n.bit_length() - d.bit_length()                     # floor(log2(n / d)) is e or e - 1
    if (n << max(-e, 0)) < (d << max(e, 0)):
        e -= 1
    if e >= 1024:
        return -math.inf if neg else math.inf
    s = min(52 - e, 1074)                                   # the result is floor(n / d * 2^s) * 2^-s
    m = (n << s) // d if s >= 0 else n // (d << -s)
    if m == 0:
        return 0.0
    v = math.ldexp(float(m), -s)                            # m < 2^53: exact
    return -v if neg else v


def bits(v):
    return struct.pack(">d", float(v)).hex()


def load_corpus():
    """(denominators, numerators per denominator, high zero limbs per numerator, GMP's 8 bytes per numerator as hex)"""
    doc = json.loads(gzip.open(os.path.join(GOLDEN, "todouble_corpus.json.gz")).read())
    den = [int(v, 16) for v in doc["den"]]
    num = [[int(v, 16) for v in row] for row in doc["num"]]
    return den, num, doc["pad"], doc["bits"]


def is_boundary(N, D):
    """N / D lies on a grid point or one unit of N next to one: N = m*D, m*D + 1 or m*D - 1"""
    return N != 0 and abs(N) % abs(D) in (0, 1, abs(D) - 1)


def padded_slab(values, pads):
    """python ints -> (signed limb counts, limbs) with pads[t] zero limbs appended above entry t"""
    lens, limbs = [], []
    for v, p in zip(values, pads):
        a, l = abs(int(v)), 0
        while a:
            limbs.append(a & (2 ** 64 - 1)); a >>= 64; l += 1
        limbs += [0] * p
        lens.append(-(l + p) if v < 0 else l + p)
    return np.array(lens, np.int32), np.array(limbs, np.uint64)


def check_corpus(lib_path, max_den_bits=None):
    """the whole corpus (or its denominators of at most max_den_bits bits) in ONE call, n = numerators per denominator,
    nrhs = denominators: every double equals GMP's, bit for bit.  At least a third of what is run lies on a boundary."""
    import slip_lu_amd as sl
    den, num, pad, want = load_corpus()
    keep = [c for c, D in enumerate(den) if max_den_bits is None or abs(D).bit_length() <= max_den_bits]
    n = len(num[0])
    boundary = sum(is_boundary(N, den[c]) for c in keep for N in num[c])
    assert 3 * boundary >= n * len(keep), (boundary, n * len(keep))
    xlen, xlimbs = padded_slab([N for c in keep for N in num[c]], [p for c in keep for p in pad[c]])
    dlen, dlimbs = padded_slab([den[c] for c in keep], [c % 2 for c in keep])      # every other denominator with a high zero limb
    got = sl.solution_to_double(n, xlen, xlimbs, dlen, dlimbs, nrhs=len(keep), lib_path=lib_path)
    assert got.shape == (len(keep), n)
    bad = [(c, t) for r, c in enumerate(keep) for t in range(n) if bits(got[r, t]) != want[c][t]]
    assert not bad, [(c, t, bits(got[keep.index(c), t]), want[c][t]) for c, t in bad[:8]]
    return len(keep) * n


def handle(lib_path, n, Ap, Ai, Alen, Alimbs, q, **kw):
    """a complete factorisation and its det = rho[n-1]"""
    import slip_lu_amd as sl
    f = sl.Factorization(n, Ap, Ai, Alen, Alimbs, q, lib_path=lib_path, **kw)
    f.run(0)
    return f, oracle_lib.bigints(*f.pivots())[-1]


def rhs_pattern(b, nrhs):
    """check_solve's right-hand sides: b, -3b + c, ..."""
    return [[int(v) for v in (b if c % 2 == 0 else -3 * b + c)] for c in range(nrhs)]


def assert_same_doubles(got, want, what):
    got, want = [bits(v) for v in got], [bits(v) for v in want]
    assert got == want, (what, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:6])


def check_reference_solutions(lib_path, name, nrhs=3, **kw):
    """solve_double of solve_rhs(n) == trunc_double of the reference's own rationals (tests/golden/solve_*), placed at q[p];
    the further right-hand sides == trunc_double of the same handle's `solve` numerators over det"""
    n, Ap, Ai, Alen, Alimbs, q, fix = solve_inputs(SOLVE_CASES[name])
    num = oracle_lib.bigints(fix["xnumlen"], fix["xnumlimbs"])
    den = oracle_lib.bigints(fix["xdenlen"], fix["xdenlimbs"])
    bs = rhs_pattern(oracle_lib.solve_rhs(n), nrhs)
    blen, blimbs = slab([v for b in bs for v in b])
    f, det = handle(lib_path, n, Ap, Ai, Alen, Alimbs, q, **kw)
    try:
        got = f.solve_double(blen, blimbs, nrhs=nrhs)
        assert f.to_double_ms() >= 0
        x = oracle_lib.bigints(*f.solve(blen, blimbs, nrhs=nrhs))
    finally:
        f.close()
    assert got.shape == (nrhs, n) and got.dtype == np.float64
    want = [0.0] * n
    for p in range(n):
        want[int(q[p])] = trunc_double(num[p], den[p])
    assert_same_doubles(got[0], want, name)
    for c in range(nrhs):
        want = [0.0] * n
        for p in range(n):
            want[int(q[p])] = trunc_double(x[c * n + p], det)
        assert_same_doubles(got[c], want, (name, c))


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
        got = f.solve_double(blen, blimbs, nrhs=nrhs, transpose=True)
        x = oracle_lib.bigints(*f.solve_transpose(blen, blimbs, nrhs=nrhs))
    finally:
        f.close()
    want = [0.0] * n
    for p in range(n):
        want[int(fix["q"][p])] = trunc_double(num[p], den[p])
    assert_same_doubles(got[0], want, name)
    for c in range(nrhs):
        assert_same_doubles(got[c], [trunc_double(x[c * n + i], det) for i in range(n)], (name, c))


def integer_rhs(n, Ap, Ai, Alen, Alimbs, q, x0):
    """b = A(:,q) x0 for x0 by position"""
    cols = columns(n, Ap, Ai, oracle_lib.bigints(Alen, Alimbs))
    b = [0] * n
    for p in range(n):
        if x0[p]:
            for i, a in cols[int(q[p])].items():
                b[i] += a * x0[p]
    return b


def check_integer_solutions(lib_path, name, **kw):
    """b = A(:,q) x0 with small integer x0 (a third of it zero, some large enough to fill 53 bits): solve_double returns
    x0 itself, as floats, at q[p] -- every quotient lies exactly on the grid, where leading bits alone land one step low"""
    n, Ap, Ai, Alen, Alimbs, q, _ = solve_inputs(SOLVE_CASES[name])
    x0 = [0 if p % 3 == 0 else ((p * 7919) % 41) - 20 for p in range(n)]
    x0[1], x0[2] = 2 ** 53 - 1, -(2 ** 52 + 1)
    blen, blimbs = slab(integer_rhs(n, Ap, Ai, Alen, Alimbs, q, x0))
    f, det = handle(lib_path, n, Ap, Ai, Alen, Alimbs, q, **kw)
    try:
        got = f.solve_double(blen, blimbs)
        slow = f.to_double_slow()
    finally:
        f.close()
    want = [0.0] * n
    for p in range(n):
        want[int(q[p])] = float(x0[p])
    assert_same_doubles(got[0], want, name)
    return slow


SCALES = [(1000, 1), (3, 7), (-1, 1), (3, -7), (2 ** 70 + 1, -(2 ** 65 + 3))]


def check_scale(lib_path, name, **kw):
    """scale = snum / sden applied before the one truncation: trunc_double(xnum * snum, det * sden), for the plain solve (as a
    pair and as a Fraction) and the transposed one; a zero scale part is SLIP_HIP_INCORRECT_INPUT"""
    import slip_lu_amd as sl
    n, Ap, Ai, Alen, Alimbs, q, _ = solve_inputs(SOLVE_CASES[name])
    bs = rhs_pattern(oracle_lib.solve_rhs(n), 2)
    blen, blimbs = slab([v for b in bs for v in b])
    f, det = handle(lib_path, n, Ap, Ai, Alen, Alimbs, q, **kw)
    try:
        x = oracle_lib.bigints(*f.solve(blen, blimbs, nrhs=2))
        xt = oracle_lib.bigints(*f.solve_transpose(blen, blimbs, nrhs=2))
        for sn, sd in SCALES:
            got = f.solve_double(blen, blimbs, nrhs=2, scale=(sn, sd))
            for c in range(2):
                want = [0.0] * n
                for p in range(n):
                    want[int(q[p])] = trunc_double(x[c * n + p] * sn, det * sd)
                assert_same_doubles(got[c], want, (name, sn, sd, c))
            got = f.solve_double(blen, blimbs, nrhs=2, transpose=True, scale=(sn, sd))
            for c in range(2):
                assert_same_doubles(got[c], [trunc_double(xt[c * n + i] * sn, det * sd) for i in range(n)], (name, "T", sn, sd, c))
        got = f.solve_double(blen, blimbs, nrhs=2, scale=Fraction(3, 7))
        assert_same_doubles(got[0], f.solve_double(blen, blimbs, nrhs=2, scale=(3, 7))[0], "Fraction")
        for bad in ((0, 1), (1, 0), (0, 0)):
            with pytest.raises(sl.SlipError) as e:
                f.solve_double(blen, blimbs, nrhs=2, scale=bad)
            assert e.value.code == -3
    finally:
        f.close()


def check_lifecycle(lib_path, name="solve_test_mat", **kw):
    """refused before the factorisation is complete, for nrhs < 1, and -- plain only -- on a handle around given factors (it holds
    no q; the transposed call works there); the same doubles after reset + run and after a GROW_X forced by a right-hand side of
    several limbs; `solve` still returns the same numerators afterwards"""
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
                f.solve_double(blen, blimbs, transpose=tr)
            assert e.value.code == -3
        f.run(0)
        with pytest.raises(sl.SlipError) as e:
            f.solve_double(blen[:0], blimbs, nrhs=0)
        assert e.value.code == -3
        det = oracle_lib.bigints(*f.pivots())[-1]
        x0 = f.solve(blen, blimbs)
        d0 = f.solve_double(blen, blimbs)
        t0 = f.solve_double(blen, blimbs, transpose=True)
        x = oracle_lib.bigints(*x0)
        want = [0.0] * n
        for p in range(n):
            want[int(q[p])] = trunc_double(x[p], det)
        assert_same_doubles(d0[0], want, "first")
        xcap = f.info()["xcap_digits"]
        dw = f.solve_double(wlen, wlimbs)                          # x needs 63 more digits than it did for b: the stride grows
        assert f.info()["xcap_digits"] > xcap
        xw = oracle_lib.bigints(*f.solve(wlen, wlimbs))
        want = [0.0] * n
        for p in range(n):
            want[int(q[p])] = trunc_double(xw[p], det)
        assert_same_doubles(dw[0], want, "wide right-hand side")
        assert_same_doubles(f.solve_double(blen, blimbs)[0], d0[0], "after the growth")
        x1 = f.solve(blen, blimbs)
        assert np.array_equal(x0[0], x1[0]) and np.array_equal(x0[1], x1[1])
        fac = f.download()
        f.reset()
        with pytest.raises(sl.SlipError):
            f.solve_double(blen, blimbs)
        f.run(0)
        assert_same_doubles(f.solve_double(blen, blimbs)[0], d0[0], "after reset + run")
        assert_same_doubles(f.solve_double(blen, blimbs, transpose=True)[0], t0[0], "transposed, after reset + run")
    finally:
        f.close()
    g = sl.Factorization.from_factors(fac, lib_path=lib_path, **{k: v for k, v in kw.items() if k in ("waves", "workers")})
    try:
        with pytest.raises(sl.SlipError) as e:
            g.solve_double(blen, blimbs)
        assert e.value.code == -3
        assert_same_doubles(g.solve_double(blen, blimbs, transpose=True)[0], t0[0], "from factors, transposed")
    finally:
        g.close()


def check_rejections(lib_path):
    """slip_hip_solution_to_double: nrhs < 1, a zero denominator, a limb array longer than its capacity"""
    import slip_lu_amd as sl
    from slip_lu_amd import _lib
    lib = _lib.load(lib_path)
    xlen, xlimbs = slab([5, -7, 2 ** 64])
    dlen, dlimbs = slab([3])
    out = np.zeros(3)
    assert [bits(v) for v in sl.solution_to_double(3, xlen, xlimbs, dlen, dlimbs, lib_path=lib_path)[0]] == \
        [bits(trunc_double(v, 3)) for v in (5, -7, 2 ** 64)]
    call = lambda n, nrhs, xcap, dl, dcap: lib.slip_hip_solution_to_double(      # noqa: E731
        n, nrhs, xlen.ctypes.data, xlimbs.ctypes.data, xcap, dl.ctypes.data, dlimbs.ctypes.data, dcap, out.ctypes.data, None)
    assert call(3, 0, xlimbs.size, dlen, 1) == -3
    assert call(3, 1, xlimbs.size - 1, dlen, 1) == -3
    assert call(3, 1, xlimbs.size, dlen, 0) == -3
    assert call(3, 1, xlimbs.size, np.zeros(1, np.int32), 1) == -3
    zlen, zlimbs = np.array([1], np.int32), np.zeros(1, np.uint64)               # one limb that is zero
    assert lib.slip_hip_solution_to_double(3, 1, xlen.ctypes.data, xlimbs.ctypes.data, xlimbs.size, zlen.ctypes.data,
                                           zlimbs.ctypes.data, 1, out.ctypes.data, None) == -3


def check_wide_handle(lib_path, name):
    """a complete factorisation whose determinant exceeds 256 digits (the wave pass's products go through memory beyond any
    register width): solve_double == trunc_double of the same handle's `solve` numerators over det, entry by entry; an
    integer solution comes back exactly"""
    entry, fix = load_case(name)
    n, q = len(fix["q"]), fix["q"]
    f, det = handle(lib_path, n, fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], q, pivot=entry["pivot"], tol=entry["tol"])
    try:
        assert det.bit_length() > 256 * 32
        b = [int(v) for v in oracle_lib.solve_rhs(n)]
        x0 = [((p * 31) % 7) - 3 for p in range(n)]
        bi = integer_rhs(n, fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], q, x0)
        blen, blimbs = slab(b + bi)
        got = f.solve_double(blen, blimbs, nrhs=2)
        x = oracle_lib.bigints(*f.solve(blen, blimbs, nrhs=2))
    finally:
        f.close()
    for c in range(2):
        want = [0.0] * n
        for p in range(n):
            want[int(q[p])] = trunc_double(x[c * n + p], det)
        assert_same_doubles(got[c], want, (name, c))
    want = [0.0] * n
    for p in range(n):
        want[int(q[p])] = float(x0[p])
    assert_same_doubles(got[1], want, (name, "integers"))
