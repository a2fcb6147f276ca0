"""Shared by tests/test_emu_tsolve.py (the emulator build) and tests/test_gpu_tsolve.py (the product on the device): the
transposed solve A(:,q)^T x = b on resident factors (slip_hip_factor_solve_transpose) and its certificate
(slip_hip_factor_check_transpose), against the reference's own rationals of A^T x = b (tests/golden/tsolve_*), the CPU
restatement on the explicitly transposed matrix, exact Python-integer residuals, and the duality c . A^-1 b formed both ways.
b goes in by pivot POSITION, x comes back by ORIGINAL row id over det = rho[n-1].  lib_path None is the product library."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import oracle_lib
import slabfile
from check_helpers import columns, duplicate_case, slab, verdict
from conftest import GOLDEN, load_case, solve_inputs

TSOLVE_CASES = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "tsolve_index.json")))}
SOLVE_CASES = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "solve_index.json")))}


def residual_t(n, cols, q, x, det, b):
    """r_k = sum_i A(i, q[k]) x[i] - det b[k]: x by row id, b by position"""
    return [sum(a * x[i] for i, a in cols[int(q[k])].items()) - det * b[k] for k in range(n)]


def handle(lib_path, n, Ap, Ai, Alen, Alimbs, q, **kw):
    """a complete factorisation and its det = rho[n-1]"""
    import slip_lu_amd as sl
    f = sl.Factorization(n, Ap, Ai, Alen, Alimbs, q, lib_path=lib_path, **kw)
    f.run(0)
    return f, oracle_lib.bigints(*f.pivots())[-1]


def tsolve(f, bs):
    """transposed solves of the right-hand sides bs (lists of n ints by position) -> the numerators by row id, per rhs"""
    n = f.n
    blen, blimbs = slab([v for b in bs for v in b])
    x = oracle_lib.bigints(*f.solve_transpose(blen, blimbs, nrhs=len(bs)))
    return [x[c * n:(c + 1) * n] for c in range(len(bs))]


def tcheck(f, bs, xs):
    blen, blimbs = slab([v for b in bs for v in b])
    xlen, xlimbs = slab([v for x in xs for v in x])
    return f.check_transpose(blen, blimbs, xlen, xlimbs, nrhs=len(bs))


def check_reference_tsolve(lib_path, name, nrhs=1, **kw):
    """b[k] = solve_rhs(n)[q[k]] with q the handle's column order: x / det is the reference's solution of A^T x = solve_rhs(n);
    further right-hand sides pass the Python-integer residual, every one passes the device certificate.  Returns the update
    queue items helper workgroups ran during the transposed solve."""
    case = TSOLVE_CASES[name]
    n, Ap, Ai, Alen, Alimbs, q, _ = solve_inputs(SOLVE_CASES[case["source"]])
    fix = slabfile.load(os.path.join(GOLDEN, name + ".slab.gz"))
    num = oracle_lib.bigints(fix["xnumlen"], fix["xnumlimbs"])
    den = oracle_lib.bigints(fix["xdenlen"], fix["xdenlimbs"])
    want = [None] * n
    for p in range(n):
        want[int(fix["q"][p])] = Fraction(num[p], den[p])
    b0 = [int(v) for v in oracle_lib.solve_rhs(n)]
    bs = [[(b0[int(q[k])] if c % 2 == 0 else -3 * b0[int(q[k])] + c) * (c // 2 + 1) for k in range(n)] for c in range(nrhs)]
    f, det = handle(lib_path, n, Ap, Ai, Alen, Alimbs, q, **kw)
    try:
        items = f.info()["farm_items"]
        xs = tsolve(f, bs)
        items = f.info()["farm_items"] - items
        ok, first, bad = tcheck(f, bs, xs)
        assert ok and list(first) == [-1] * nrhs and list(bad) == [0] * nrhs
    finally:
        f.close()
    assert [Fraction(v, det) for v in xs[0]] == want
    cols = columns(n, Ap, Ai, oracle_lib.bigints(Alen, Alimbs))
    for c in range(1, nrhs):
        assert not any(residual_t(n, cols, q, xs[c], det, bs[c])), c
    return items


def transpose_csc(n, Ap, Ai, vals):
    """A^T as CSC (Ap, Ai, values), a row repeated in a column of A kept once, with its LAST value"""
    ent = {}
    for j in range(n):
        for p in range(int(Ap[j]), int(Ap[j + 1])):
            ent[(int(Ai[p]), j)] = vals[p]
    tcols = [[] for _ in range(n)]
    for (i, j), v in sorted(ent.items()):
        tcols[i].append((j, v))
    TAp = np.cumsum([0] + [len(c) for c in tcols]).astype(np.int64)
    TAi = np.array([j for c in tcols for j, _ in c], np.int32)
    return TAp, TAi, [v for c in tcols for _, v in c]


def check_cpu_restatement(lib_path, n=300, density=0.02, bits=20, seed=11):
    """int64 b: the canonical fractions equal orc_solve on the explicitly transposed matrix; two-limb b: A(:,q)^T xnum ==
    det b with Python integers; the numerators are linear in b"""
    import slip_lu_amd as sl
    Ap, Ai, Ax = oracle_lib.matgen(n, density, bits, seed)
    Alen, Alimbs = sl.ints_to_slab(Ax)
    q = np.random.RandomState(seed).permutation(n).astype(np.int32)
    rng = np.random.default_rng(seed)
    b1 = [int(v) for v in rng.integers(-10 ** 6, 10 ** 6, n)]
    b2 = [int(rng.integers(-2 ** 62, 2 ** 62)) * int(rng.integers(1, 2 ** 62)) * (k % 3 != 0) for k in range(n)]     # 2 limbs, 1/3 zeros
    b3 = [u + v for u, v in zip(b1, b2)]
    f, det = handle(lib_path, n, Ap, Ai, Alen, Alimbs, q)
    try:
        x1, x2, x3 = tsolve(f, [b1, b2, b3])
    finally:
        f.close()
    assert [u + v for u, v in zip(x1, x2)] == x3
    vals = [int(v) for v in Ax]
    cols = columns(n, Ap, Ai, vals)
    for x, b in ((x1, b1), (x2, b2)):
        assert not any(residual_t(n, cols, q, x, det, b))
    # A(:,q)^T x = b1  <=>  A^T x = b_orig with b_orig[q[k]] = b1[k]; orc_solve's numerators are by ITS positions (qT)
    b_orig = np.zeros(n, np.int64)
    b_orig[q] = b1
    TAp, TAi, tvals = transpose_csc(n, Ap, Ai, vals)
    Tlen, Tlimbs = sl.ints_to_slab(np.array(tvals, np.int64))
    qT = np.arange(n, dtype=np.int32)
    want, detT = oracle_lib.factorize_and_solve(n, TAp, TAi, Tlen, Tlimbs, qT, b_orig)
    for p in range(n):
        assert Fraction(x1[int(qT[p])], det) == Fraction(want[p], detT), p


def check_duality(lib_path, name):
    """y = solve(b) by position, z = solve_transpose(c) by row id: c . y == z . b exactly (both are det * c^T A(:,q)^-1 b);
    the certificate accepts z"""
    entry, fix = load_case(name)
    n, q = len(fix["q"]), fix["q"]
    f, det = handle(lib_path, n, fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], q, pivot=entry["pivot"], tol=entry["tol"])
    try:
        b = [int(v) for v in oracle_lib.solve_rhs(n)]
        c = [((k * 40503) % 1999) - 999 for k in range(n)]
        blen, blimbs = slab(b)
        y = oracle_lib.bigints(*f.solve(blen, blimbs))
        z, = tsolve(f, [c])
        ok, first, bad = tcheck(f, [c], [z])
        assert ok and list(first) == [-1] and list(bad) == [0], (name, first, bad)
    finally:
        f.close()
    assert any(z)
    assert sum(u * v for u, v in zip(c, y)) == sum(u * v for u, v in zip(z, b)), name


def check_verdicts(lib_path, name):
    """clean transposed solves pass; one numerator +1, the numerators over 2*det, a swapped pair are found at the first
    position and with the count the Python-integer residual gives; the other right-hand sides stay clean"""
    _, fix = load_case(name)
    n, Ap, Ai, Alen, Alimbs, q = len(fix["q"]), fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"]
    b0 = [int(v) for v in oracle_lib.solve_rhs(n)]
    bs = [b0, [(3 * v - 7) * (2 ** 70 + 12345) if k % 4 else 0 for k, v in enumerate(b0)], [-v + 1 for v in b0]]
    f, det = handle(lib_path, n, Ap, Ai, Alen, Alimbs, q)
    try:
        xs = tsolve(f, bs)
        for nrhs in (1, 3):
            ok, first, bad = tcheck(f, bs[:nrhs], xs[:nrhs])
            assert ok and list(first) == [-1] * nrhs and list(bad) == [0] * nrhs
        cols = columns(n, Ap, Ai, oracle_lib.bigints(Alen, Alimbs))
        x = xs[1]
        nz = [i for i, v in enumerate(x) if v]
        i0 = max(nz, key=lambda i: (abs(x[i]).bit_length(), i))
        a, b = next((s, t) for s in nz for t in nz if x[s] != x[t])
        plus = list(x); plus[i0] += 1
        swapped = list(x); swapped[a], swapped[b] = x[b], x[a]
        for label, y in (("plus one", plus), ("over 2 det", [2 * v for v in x]), ("swapped", swapped)):
            want_first, want_bad = verdict(residual_t(n, cols, q, y, det, bs[1]))
            assert want_bad > 0, label
            ok, first, bad = tcheck(f, bs, [xs[0], y, xs[2]])
            assert not ok, label
            assert list(first) == [-1, want_first, -1] and list(bad) == [0, want_bad, 0], (label, first, bad)
    finally:
        f.close()


def check_rejections(lib_path):
    """every rejected input of the transposed check and solve is SLIP_HIP_INCORRECT_INPUT (-3)"""
    import slip_lu_amd as sl
    from slip_lu_amd import _lib
    _, fix = load_case("test_mat")
    n, Ap, Ai, Alen, Alimbs, q = len(fix["q"]), fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"]
    b = [int(v) for v in oracle_lib.solve_rhs(n)]
    lib = _lib.load(lib_path)
    first, bad = np.zeros(1, np.int32), np.zeros(1, np.int64)
    f, det = handle(lib_path, n, Ap, Ai, Alen, Alimbs, q)
    try:
        x, = tsolve(f, [b])
        blen, blimbs = slab(b)
        xlen, xlimbs = slab(x)
        with pytest.raises(sl.SlipError) as e:                     # nrhs = 0
            f.check_transpose(blen[:0], blimbs, xlen[:0], xlimbs, nrhs=0)
        assert e.value.code == -3
        for bcap, xcap in ((blimbs.size - 1, xlimbs.size), (blimbs.size, xlimbs.size - 1)):    # a capacity short of the counts
            assert lib.slip_hip_factor_check_transpose(f.h, 1, blen.ctypes.data, blimbs.ctypes.data, bcap, xlen.ctypes.data,
                                                       xlimbs.ctypes.data, xcap, first.ctypes.data, bad.ctypes.data, None) == -3
        fac = f.download()
    finally:
        f.close()
    g = sl.Factorization.from_factors(fac, lib_path=lib_path)       # no A behind this handle: no certificate
    try:
        with pytest.raises(sl.SlipError) as e:
            g.check_transpose(blen, blimbs, xlen, xlimbs)
        assert e.value.code == -3
    finally:
        g.close()
    h = sl.Factorization(n, Ap, Ai, Alen, Alimbs, q, lib_path=lib_path)
    try:
        h.run(n // 2)                                               # an incomplete factorisation
        for call in (lambda: h.solve_transpose(blen, blimbs), lambda: h.check_transpose(blen, blimbs, xlen, xlimbs)):
            with pytest.raises(sl.SlipError) as e:
                call()
            assert e.value.code == -3
    finally:
        h.close()


def check_duplicates(lib_path):
    """column 1 holds row 2 twice (5, then -3): the certificate tests the factorised matrix, which keeps -3"""
    n, Ap, Ai, Alen, Alimbs, x0, _, _ = duplicate_case()
    q = np.arange(n, dtype=np.int32)
    f, det = handle(lib_path, n, Ap, Ai, Alen, Alimbs, q)
    try:
        x = [det * v for v in x0]
        last = [sum(a * x0[i] for i, a in col.items()) for col in columns(n, Ap, Ai, oracle_lib.bigints(Alen, Alimbs))]
        summed = list(last); summed[1] += 5 * x0[2]
        for b, want in ((last, (True, -1, 0)), (summed, (False, 1, 1))):
            ok, first, bad = tcheck(f, [b], [x])
            assert (ok, int(first[0]), int(bad[0])) == want
        z, = tsolve(f, [last])
        assert z == x
    finally:
        f.close()


def check_lifecycle(lib_path, name="solve_gen_n40", **kw):
    """refused on an incomplete factorisation and after reset; the same answer after run again; the plain solve is
    bit-identical before and after transposed solves on the handle (x, its row tags and the ticket counter are shared); a
    handle around the downloaded factors gives the same numerators; all-zero and single-nonzero right-hand sides"""
    import slip_lu_amd as sl
    n, Ap, Ai, Alen, Alimbs, q, _ = solve_inputs(SOLVE_CASES[name])
    b = [int(v) for v in oracle_lib.solve_rhs(n)]
    c = [((k * 7) % 23) - 11 for k in range(n)]
    e3 = [0] * n; e3[3] = -7
    blen, blimbs = slab(b)
    clen, climbs = slab(c)
    f = sl.Factorization(n, Ap, Ai, Alen, Alimbs, q, lib_path=lib_path, **kw)
    try:
        f.run(n // 2)
        with pytest.raises(sl.SlipError):
            f.solve_transpose(clen, climbs)
        f.run(0)
        det = oracle_lib.bigints(*f.pivots())[-1]
        y0 = f.solve(blen, blimbs)
        z0 = f.solve_transpose(clen, climbs)
        ms, view_ms = f.solve_transpose_ms()
        assert ms >= 0 and view_ms >= 0
        z1 = f.solve_transpose(clen, climbs)
        assert f.solve_transpose_ms()[1] == 0                      # the view is reused
        y1 = f.solve(blen, blimbs)
        for u, v in zip(y0 + z0, y1 + z1):
            assert np.array_equal(u, v)
        zs = tsolve(f, [[0] * n, e3, [0] * n])
        assert zs[0] == [0] * n and zs[2] == [0] * n
        cols = columns(n, Ap, Ai, oracle_lib.bigints(Alen, Alimbs))
        assert any(zs[1]) and not any(residual_t(n, cols, q, zs[1], det, e3))
        fac = f.download()
        f.reset()
        with pytest.raises(sl.SlipError):
            f.solve_transpose(clen, climbs)
        f.run(0)
        z2 = f.solve_transpose(clen, climbs)
        assert np.array_equal(z0[0], z2[0]) and np.array_equal(z0[1], z2[1])
    finally:
        f.close()
    g = sl.Factorization.from_factors(fac, lib_path=lib_path, **{k: v for k, v in kw.items() if k in ("waves", "workers")})
    try:
        z3 = g.solve_transpose(clen, climbs)
    finally:
        g.close()
    assert oracle_lib.bigints(*z3) == oracle_lib.bigints(*z0)

