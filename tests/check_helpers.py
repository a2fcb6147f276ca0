"""Shared by tests/test_emu_check.py (the emulator build) and tests/test_gpu_check.py (the product on the device): inputs
of the exact solution check (slip_hip_factor_check, slip_hip_check_solution) and its expected verdicts, computed with
exact Python integers.  lib_path None is the product library."""
import json
import os
import random
from fractions import Fraction
from math import lcm

import numpy as np
import pytest

import oracle_lib
from conftest import GOLDEN, load_case, solve_inputs

SOLVE_CASES = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "solve_index.json")))}


def slab(values):
    """python ints -> (signed limb counts, limbs)"""
    lens, limbs = [], []
    for v in values:
        a, n = abs(int(v)), 0
        while a:
            limbs.append(a & (2 ** 64 - 1)); a >>= 64; n += 1
        lens.append(-n if v < 0 else n)
    return np.array(lens, np.int32), np.array(limbs, np.uint64)


def columns(n, Ap, Ai, vals):
    """column j -> {row: value}, a repeated row keeping its LAST value (what slip_hip_factor_create factorises)"""
    cols = [dict() for _ in range(n)]
    for j in range(n):
        for p in range(int(Ap[j]), int(Ap[j + 1])):
            cols[j][int(Ai[p])] = vals[p]
    return cols


def residual(n, cols, xcol, d, b):
    """r_i = sum_j A(i,j) x_j - d b_i"""
    r = [-d * v for v in b]
    for j in range(n):
        if xcol[j]:
            for i, a in cols[j].items():
                r[i] += a * xcol[j]
    return r


def verdict(r):
    bad = [i for i, v in enumerate(r) if v != 0]
    return (bad[0] if bad else -1), len(bad)


def factor_and_solve(lib_path, n, Ap, Ai, Alen, Alimbs, q, bs):
    """a complete handle and its solve of the right-hand sides bs (lists of n ints): (handle, x by position, det)"""
    import slip_lu_amd as sl
    f = sl.Factorization(n, Ap, Ai, Alen, Alimbs, q, lib_path=lib_path)
    f.run(0)
    rholen, rholimbs = f.pivots()
    det = oracle_lib.bigints(rholen, rholimbs)[-1]
    blen, blimbs = slab([v for b in bs for v in b])
    xlen, xlimbs = f.solve(blen, blimbs, nrhs=len(bs))
    return f, oracle_lib.bigints(xlen, xlimbs), det


def rhs_pair(n):
    b0 = [int(v) for v in oracle_lib.solve_rhs(n)]
    b1 = [(3 * v - 7) * (2 ** 70 + 12345) if i % 4 else 0 for i, v in enumerate(b0)]      # multi-limb, some zeros
    b2 = [-v + 1 for v in b0]
    return [b0, b1, b2]


def check_clean(f, n, x, bs):
    """the solve's own numerators pass, for the first right-hand side alone and for all of them"""
    for nrhs in (1, len(bs)):
        blen, blimbs = slab([v for b in bs[:nrhs] for v in b])
        xlen, xlimbs = slab(x[:nrhs * n])
        ok, first, bad = f.check(blen, blimbs, xlen, xlimbs, nrhs=nrhs)
        assert ok and list(first) == [-1] * nrhs and list(bad) == [0] * nrhs
        assert f.check_ms() >= 0


def perturbations(xs, rng):
    """(label, perturbed copy) of one right-hand side's numerators"""
    nz = [p for p, v in enumerate(xs) if v]
    p = max(nz, key=lambda t: (abs(xs[t]).bit_length(), t))
    L = (abs(xs[p]).bit_length() + 63) // 64
    out = []
    y = list(xs); y[p] += 1; out.append(("plus one", y))
    y = list(xs); y[p] = (-1 if y[p] < 0 else 1) * (abs(y[p]) ^ ((2 ** 64 - 1) << (64 * (L - 1)))); out.append(("high limb flipped", y))
    y = list(xs); y[p] += 2 ** (64 * (L + 3)); out.append(("far above every width", y))
    y = list(xs); y[rng.choice(nz)] = 0; out.append(("zeroed", y))
    a, b = next((s, t) for s in nz for t in nz if xs[s] != xs[t])
    y = list(xs); y[a], y[b] = y[b], y[a]; out.append(("swapped", y))
    return out


def check_perturbations(f, n, Ap, Ai, Alen, Alimbs, q, x, det, bs):
    """every perturbation of the middle right-hand side of three is found exactly where the exact residual says; the
    other two stay clean"""
    cols = columns(n, Ap, Ai, oracle_lib.bigints(Alen, Alimbs))
    rng = random.Random(n)
    blen, blimbs = slab([v for b in bs for v in b])
    for label, y in perturbations(x[n:2 * n], rng):
        xcol = [0] * n
        for p in range(n):
            xcol[int(q[p])] = y[p]
        want_first, want_bad = verdict(residual(n, cols, xcol, det, bs[1]))
        assert want_bad > 0, label
        xlen, xlimbs = slab(x[:n] + y + x[2 * n:])
        ok, first, bad = f.check(blen, blimbs, xlen, xlimbs, nrhs=3)
        assert not ok, label
        assert list(first) == [-1, want_first, -1], label
        assert list(bad) == [0, want_bad, 0], label


def reference_rationals(case):
    """A, b and the reference's own solution of a solve golden, brought to one denominator in ORIGINAL column order"""
    n, Ap, Ai, Alen, Alimbs, q, fix = solve_inputs(case)
    num = oracle_lib.bigints(fix["xnumlen"], fix["xnumlimbs"])
    den = oracle_lib.bigints(fix["xdenlen"], fix["xdenlimbs"])
    fr = [Fraction(a, b) for a, b in zip(num, den)]
    d = lcm(*[v.denominator for v in fr])
    xcol = [0] * n
    for p in range(n):
        xcol[int(q[p])] = int(fr[p] * d)
    return n, Ap, Ai, Alen, Alimbs, [int(v) for v in oracle_lib.solve_rhs(n)], xcol, d


def check_reference_rationals(lib_path, name):
    import slip_lu_amd as sl
    n, Ap, Ai, Alen, Alimbs, b, xcol, d = reference_rationals(SOLVE_CASES[name])
    blen, blimbs = slab(b)
    xlen, xlimbs = slab(xcol)
    for dd, want in ((d, True), (d + 1, False)):
        dlen, dlimbs = slab([dd])
        ok, first, bad = sl.check_solution(n, Ap, Ai, Alen, Alimbs, blen, blimbs, xlen, xlimbs, dlen, dlimbs, lib_path=lib_path)
        assert ok == want, (name, dd)
        if want:
            assert list(first) == [-1] and list(bad) == [0]
        else:
            vals = oracle_lib.bigints(Alen, Alimbs)
            assert (int(first[0]), int(bad[0])) == verdict(residual(n, columns(n, Ap, Ai, vals), xcol, dd, b))


def wide_case(n, ylimbs, nrhs, seed):
    """a random sparse A with 1-3 limb entries and y of about `ylimbs` limbs: b = A y, x = d_c y for d_c of 1, 7 and a
    multi-limb value in turn"""
    rng = random.Random(seed)
    Ap, Ai, vals = [0], [], []
    for j in range(n):
        rows = sorted(rng.sample(range(n), rng.randint(1, 4)))
        for i in rows:
            Ai.append(i)
            vals.append(rng.choice((-1, 1)) * rng.getrandbits(64 * rng.randint(1, 3)) | 1)
        Ap.append(len(Ai))
    cols = columns(n, Ap, Ai, vals)
    dens = [1, 7, -(2 ** 100 + 3)]
    bs, xs, ds = [], [], []
    for c in range(nrhs):
        y = [rng.choice((-1, 1)) * rng.getrandbits(64 * ylimbs - rng.randint(0, 100)) for _ in range(n)]
        d = dens[c % len(dens)]
        bs.append(residual(n, cols, y, 0, [0] * n))
        xs.append([d * v for v in y])
        ds.append(d)
    Alen, Alimbs = slab(vals)
    return n, np.array(Ap, np.int64), np.array(Ai, np.int32), Alen, Alimbs, cols, bs, xs, ds


def check_wide(lib_path, n, ylimbs, nrhs, seed):
    import slip_lu_amd as sl
    n, Ap, Ai, Alen, Alimbs, cols, bs, xs, ds = wide_case(n, ylimbs, nrhs, seed)
    blen, blimbs = slab([v for b in bs for v in b])
    dlen, dlimbs = slab(ds)
    xlen, xlimbs = slab([v for x in xs for v in x])
    ok, first, bad = sl.check_solution(n, Ap, Ai, Alen, Alimbs, blen, blimbs, xlen, xlimbs, dlen, dlimbs, nrhs=nrhs, lib_path=lib_path)
    assert ok and list(first) == [-1] * nrhs and list(bad) == [0] * nrhs
    # the top limb of one x flipped: reported at the rows of its column
    c, j = nrhs - 1, n // 2
    v = xs[c][j]
    L = (abs(v).bit_length() + 63) // 64
    y = list(xs[c]); y[j] = (-1 if v < 0 else 1) * (abs(v) ^ ((2 ** 64 - 1) << (64 * (L - 1))))
    want = verdict(residual(n, cols, y, ds[c], bs[c]))
    xlen, xlimbs = slab([v for x in xs[:c] for v in x] + y)
    ok, first, bad = sl.check_solution(n, Ap, Ai, Alen, Alimbs, blen, blimbs, xlen, xlimbs, dlen, dlimbs, nrhs=nrhs, lib_path=lib_path)
    assert not ok
    assert list(first) == [-1] * c + [want[0]] and list(bad) == [0] * c + [want[1]]


def duplicate_case():
    """column 1 holds row 2 twice (5, then -3): the factorised matrix keeps -3"""
    n = 3
    Ap = np.array([0, 2, 5, 6], np.int64)
    Ai = np.array([0, 1, 2, 0, 2, 2], np.int32)
    vals = [4, 1, 5, 2, -3, 9]
    Alen, Alimbs = slab(vals)
    x = [1, -2, 3]
    last = residual(n, columns(n, Ap, Ai, vals), x, 0, [0] * n)
    summed = list(last); summed[2] += 5 * x[1]
    return n, Ap, Ai, Alen, Alimbs, x, last, summed


def check_duplicates(lib_path):
    import slip_lu_amd as sl
    n, Ap, Ai, Alen, Alimbs, x, last, summed = duplicate_case()
    xlen, xlimbs = slab(x)
    dlen, dlimbs = slab([1])
    for b, want in ((last, True), (summed, False)):
        blen, blimbs = slab(b)
        ok, first, bad = sl.check_solution(n, Ap, Ai, Alen, Alimbs, blen, blimbs, xlen, xlimbs, dlen, dlimbs, lib_path=lib_path)
        assert ok == want
        assert (int(first[0]), int(bad[0])) == ((-1, 0) if want else (2, 1))


def check_error_paths(lib_path):
    """every rejected input is SLIP_HIP_INCORRECT_INPUT (-3)"""
    import slip_lu_amd as sl
    from slip_lu_amd import _lib
    _, fix = load_case("test_mat")
    n, Ap, Ai, Alen, Alimbs, q = len(fix["q"]), fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"]
    b = [int(v) for v in oracle_lib.solve_rhs(n)]
    f, x, det = factor_and_solve(lib_path, n, Ap, Ai, Alen, Alimbs, q, [b])
    blen, blimbs = slab(b)
    xlen, xlimbs = slab(x)
    lib = _lib.load(lib_path)
    first, bad = np.zeros(1, np.int32), np.zeros(1, np.int64)
    try:
        with pytest.raises(sl.SlipError) as e:                     # nrhs = 0
            f.check(blen[:0], blimbs, xlen[:0], xlimbs, nrhs=0)
        assert e.value.code == -3
        # a capacity shorter than the limbs the counts promise, for b and for x
        assert lib.slip_hip_factor_check(f.h, 1, blen.ctypes.data, blimbs.ctypes.data, blimbs.size - 1, xlen.ctypes.data,
                                         xlimbs.ctypes.data, xlimbs.size, first.ctypes.data, bad.ctypes.data, None) == -3
        assert lib.slip_hip_factor_check(f.h, 1, blen.ctypes.data, blimbs.ctypes.data, blimbs.size, xlen.ctypes.data,
                                         xlimbs.ctypes.data, xlimbs.size - 1, first.ctypes.data, bad.ctypes.data, None) == -3
        fac = f.download()
    finally:
        f.close()
    # d = 0, and a short d capacity
    xcol = [0] * n
    for p in range(n):
        xcol[int(q[p])] = x[p]
    xclen, xclimbs = slab(xcol)
    with pytest.raises(sl.SlipError) as e:
        sl.check_solution(n, Ap, Ai, Alen, Alimbs, blen, blimbs, xclen, xclimbs, np.zeros(1, np.int32), np.zeros(0, np.uint64), lib_path=lib_path)
    assert e.value.code == -3
    dlen, dlimbs = slab([det])
    Ap_, Ai_ = np.ascontiguousarray(Ap, np.int64), np.ascontiguousarray(Ai, np.int32)
    Alen_, Alimbs_ = np.ascontiguousarray(Alen, np.int32), np.ascontiguousarray(Alimbs, np.uint64)
    assert lib.slip_hip_check_solution(n, Ap_.ctypes.data, Ai_.ctypes.data, Alen_.ctypes.data, Alimbs_.ctypes.data, 1,
                                       blen.ctypes.data, blimbs.ctypes.data, blimbs.size, xclen.ctypes.data, xclimbs.ctypes.data,
                                       xclimbs.size, dlen.ctypes.data, dlimbs.ctypes.data, dlimbs.size - 1,
                                       first.ctypes.data, bad.ctypes.data, None) == -3
    ok, _, _ = sl.check_solution(n, Ap, Ai, Alen, Alimbs, blen, blimbs, xclen, xclimbs, dlen, dlimbs, lib_path=lib_path)
    assert ok                                                    # the same call with the right capacity
    # a handle around given factors holds no A
    g = sl.Factorization.from_factors(fac, lib_path=lib_path)
    try:
        with pytest.raises(sl.SlipError) as e:
            g.check(blen, blimbs, xlen, xlimbs)
        assert e.value.code == -3
    finally:
        g.close()
    # an incomplete factorisation
    h = sl.Factorization(n, Ap, Ai, Alen, Alimbs, q, lib_path=lib_path)
    try:
        h.run(n // 2)
        with pytest.raises(sl.SlipError) as e:
            h.check(blen, blimbs, xlen, xlimbs)
        assert e.value.code == -3
    finally:
        h.close()
