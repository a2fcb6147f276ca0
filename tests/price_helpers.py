"""Shared by tests/test_emu_price.py (the emulator build) and tests/test_gpu_price.py (the product on the device): exact
pricing fused on the device (slip_hip_factor_price).  The oracle is twofold for every call: (a) Python integers and
fractions -- ynum from the handle's own solve_transpose (pinned to goldens elsewhere), X and A from the host columns of M, the
selection from ratio_helpers.oracle_ties / pick with dsign = sign(det) -- and (b) the three-call route on the device
(solve_transpose + SparseMatrix.multiply + ratio_test) on the same operands.  Every comparison is exact equality.  lib_path
None is the product library."""
import ctypes as C
import random
from fractions import Fraction

import numpy as np
import pytest

import oracle_lib
from check_helpers import columns, slab
from conftest import load_case
from product_helpers import Mat, digits, same_slab
from ratio_helpers import handle_problems, oracle_ties, pick

B = 2 ** 32
COMBOS = ((1, False), (1, True), (-1, False), (-1, True))       # (sense, with key)


def sign(v):
    return (v > 0) - (v < 0)


# ---- the handle and the candidate columns ----

class Case:
    """a complete handle on a golden; negative: one column negated when the golden's det is positive (the pivot search goes
    by magnitude, so the same pivots are chosen and det changes sign: ratio_helpers.check_negative_det)"""

    def __init__(self, lib_path, name, negative=False, **kw):
        import slip_lu_amd as sl
        _, fix = load_case(name)
        self.lib_path, self.kw = lib_path, kw
        self.n, self.Ap, self.Ai, self.Alimbs, self.q = len(fix["q"]), fix["Ap"], fix["Ai"], fix["Alimbs"], fix["q"]
        self.Alen = np.array(fix["Alen"], np.int32).copy()
        self.f = sl.Factorization(self.n, self.Ap, self.Ai, self.Alen, self.Alimbs, self.q, lib_path=lib_path, **kw)
        self.f.run(0)
        self.det = oracle_lib.bigints(*self.f.pivots())[-1]
        if negative and self.det > 0:
            self.f.close()
            j = int(self.q[0])
            self.Alen[int(self.Ap[j]):int(self.Ap[j + 1])] *= -1
            self.f = sl.Factorization(self.n, self.Ap, self.Ai, self.Alen, self.Alimbs, self.q, lib_path=lib_path, **kw)
            self.f.run(0)
            self.det = oracle_lib.bigints(*self.f.pivots())[-1]
        self.cols = columns(self.n, self.Ap, self.Ai, oracle_lib.bigints(self.Alen, self.Alimbs))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.f.close()


def shifted(n, cols, count):
    """count candidate columns: column j is column j % n of A moved by 1 + j // n rows (a column of A itself is in the basis)"""
    return [[((i - 1 - j // n) % n, v) for i, v in cols[j % n].items()] for j in range(count)]


def random_columns(n, count, seed):
    rng = random.Random(seed)
    return [[(i, rng.randrange(-9, 10)) for i in rng.sample(range(n), rng.randrange(1, min(n, 5) + 1))] for _ in range(count)]


def small_rhs(n, count, seed, span=9):
    rng = random.Random(seed)
    return [[rng.randrange(-span, span + 1) for _ in range(n)] for _ in range(count)]


def small_costs(ncols, nprob, seed):
    rng = random.Random(seed)
    return [[rng.randrange(-20, 21) for _ in range(ncols)] for _ in range(nprob)]


# ---- the oracle ----

def values(mat, n, y, det, nprob, nside, gs):
    """(X, A) per problem from M's host columns and the numerators y (flat, by row id): A is None with nside = 1"""
    out = []
    for c in range(nprob):
        yx = y[nside * c * n:(nside * c + 1) * n]
        X = [sum(v * yx[i] for i, v in col.items()) - (det * gs[c][j] if gs is not None else 0) for j, col in enumerate(mat.last)]
        A = None
        if nside == 2:
            ya = y[(2 * c + 1) * n:(2 * c + 2) * n]
            A = [sum(v * ya[i] for i, v in col.items()) for col in mat.last]
        out.append((X, A))
    return out


def widths(mat, n, y, det, nvec, nside, gs):
    """W of every item as slip_product_kernel derives it: max(max_e(|a_e| + |y_e|), |det| + |g_j|) + 1 (the a side's g is empty)"""
    out = []
    for v in range(nvec):
        yv = y[v * n:(v + 1) * n]
        for j, col in enumerate(mat.last):
            w = max([digits(a) + digits(yv[i]) for i, a in col.items()] + [0])
            if gs is not None:
                w = max(w, digits(det) + (digits(gs[v // nside][j]) if v % nside == 0 else 0))
            out.append(w + 1)
    return out


def selection(vals, det, nside, sense, key):
    """per problem (best, nties, neligible, vsign) and the flat winners (X_best, A_best or 0; zeros with best = -1)"""
    dsign = sign(det)
    res, win = [], []
    for X, A in vals:
        if nside == 2:
            fr = [Fraction(x, a) if a else None for x, a in zip(X, A)]
            best, nties, nelig = pick(*oracle_ties(X, A, sense, dsign, fr), key)
        else:
            best, nties, nelig = pick(*oracle_ties(X, None, sense * dsign), key)      # the smallest sense * X_j / det
        res.append((best, nties, nelig, sign(X[best]) * dsign if best >= 0 else 0))
        win += [X[best] if best >= 0 else 0, A[best] if best >= 0 and nside == 2 else 0]
    return res, win


def check_price(case, dev, mat, bvecs, nprob, nside, gs=None, combos=COMBOS, plain=True, inspect=None):
    """one set of operands under every combination: price against the oracle and against the three-call route; returns the
    sum of the path counts.  inspect(vals, y): the caller's assertions on the oracle's (X, A) and ynum, before price is called"""
    import slip_lu_amd as sl
    f, n, det, ncols, nvec = case.f, case.n, case.det, mat.ncols, nside * nprob
    dsign = sign(det)
    assert len(bvecs) == nvec
    b = slab([v for bb in bvecs for v in bb])
    cost = slab([v for g in gs for v in g]) if gs is not None else None
    # call 1 of the three-call route, and the oracle's ynum
    ylen, ylimbs = f.solve_transpose(*b, nrhs=nvec)
    y = oracle_lib.bigints(ylen, ylimbs)
    vals = values(mat, n, y, det, nprob, nside, gs)
    if inspect:
        inspect(vals, y)
    # call 2: r = M^T y - det g, the a sides with an empty g
    if gs is not None:
        gfull = [v for c in range(nprob) for side in range(nside) for v in (gs[c] if side == 0 else [0] * ncols)]
        r = dev.multiply(ylen, ylimbs, nvec=nvec, transpose=True, b=slab(gfull), d=slab([det] * nvec))
    else:
        r = dev.multiply(ylen, ylimbs, nvec=nvec, transpose=True)
    flat = [v for X, A in vals for side in ((X, A) if nside == 2 else (X,)) for v in side]
    same_slab(r, flat, "the products of the three-call route")
    # (the handle-less ratio test knows no det: both sides times its sign are the true values times |det|)
    x3 = slab([dsign * v for X, _ in vals for v in X])
    a3 = slab([dsign * v for _, A in vals for v in A]) if nside == 2 else (None, None)
    karr = np.array([(7 * j) % 5 for j in range(ncols)], np.int32)
    total = [0, 0, 0, 0]
    for sense, with_key in combos:
        key = karr if with_key else None
        want, win = selection(vals, det, nside, sense, key)
        got = f.price(dev, *b, nprob=nprob, sides=nside, cost=cost, sense=sense, key=key, winners=True)
        assert [tuple(int(got[t][c]) for t in range(4)) for c in range(nprob)] == want, (nside, sense, with_key)
        same_slab(got[4:], win, "the winners' numerators")
        three = sl.ratio_test(ncols, *x3, *a3, nprob=nprob, sense=sense, key=key, lib_path=case.lib_path)      # call 3
        assert [tuple(int(three[t][c]) for t in range(3)) for c in range(nprob)] == [w[:3] for w in want], (nside, sense, with_key)
        paths = f.price_paths()
        assert paths[0] == sum(w[2] for w in want) and paths[1] >= sum(w[1] for w in want)
        ms = f.price_ms()
        assert len(ms) == 4 and all(v >= 0 for v in ms)
        total = [u + v for u, v in zip(total, paths)]
        if plain:                                                  # without the winners' slab: the same four arrays
            four = f.price(dev, *b, nprob=nprob, sides=nside, cost=cost, sense=sense, key=key)
            assert len(four) == 4 and all(np.array_equal(u, v) for u, v in zip(four, got[:4]))
    return total


# ---- 1. geometry: the 64-entry rounds of the bound pass, the 64-candidate chunks ----

def check_geometry(lib_path, sizes=(1, 63, 64, 65, 130), shapes=((1, 1), (1, 2), (3, 1), (3, 2)), name="gen_n40", light=False, **kw):
    """(nprob, nside) in shapes on every ncols; light, for the emulator: one combination of (sense, key) each, taken in turn"""
    with Case(lib_path, name, **kw) as case:
        n = case.n
        bvecs = small_rhs(n, 6, 21)
        for ncols in sizes:
            mat = Mat(n, ncols, shifted(n, case.cols, ncols))
            dev = mat.device(lib_path)
            try:
                for t, (nprob, nside) in enumerate(shapes):
                    gs = small_costs(ncols, nprob, 22 + ncols) if t % 2 == 0 else None
                    check_price(case, dev, mat, bvecs[:nside * nprob], nprob, nside, gs, COMBOS[(t + ncols) % 4:][:1] if light else COMBOS,
                                plain=False)
            finally:
                dev.close()


# ---- 2. shapes of M ----

def check_shapes(lib_path, name="gen_n40", combos=COMBOS, **kw):
    with Case(lib_path, name, **kw) as case:
        n, q, det, f = case.n, case.q, case.det, case.f
        ks = [n // 4, n - 2, n // 4, 1]                             # copies of basis columns A(:, q[k]), one of them twice
        cols = [[(3 % n, 99), (5 % n, 2), (3 % n, -4)], [], [(1, 0), (2, 7)]] + [list(case.cols[int(q[k])].items()) for k in ks]
        cols += shifted(n, case.cols, 6) + random_columns(n, 3, 31)
        mat = Mat(n, len(cols), cols)
        assert not mat.last[1] and len(mat.cols[0]) == len(mat.last[0]) + 1 and mat.last[0][3 % n] == -4 and 0 in mat.last[2].values()
        ncols = mat.ncols
        bvecs = small_rhs(n, 4, 32)
        # problem 0: g_j = b[k] on the copies, 0 on the empty column -- X_j is exactly 0 there; every other column is moved to
        # X_j / det >= 1 by its g_j, so with sense +1 the minimum is 0 and exactly these five columns tie
        y = oracle_lib.bigints(*f.solve_transpose(*slab(bvecs[0])))
        S = [sum(v * y[i] for i, v in col.items()) for col in mat.last]
        g0 = [S[j] // det - 1 for j in range(ncols)]
        g0[1] = 0
        for t, k in enumerate(ks):
            g0[3 + t] = bvecs[0][k]
        g1 = small_costs(ncols, 1, 33)[0]
        g1[1] = 5
        dev = mat.device(lib_path)
        try:
            vals = values(mat, n, y + oracle_lib.bigints(*f.solve_transpose(*slab(bvecs[1]))), det, 2, 1, [g0, g1])
            assert [vals[0][0][j] for j in (1, 3, 4, 5, 6)] == [0] * 5 and vals[1][0][1] == -5 * det
            karr = np.array([(7 * j) % 5 for j in range(ncols)], np.int32)
            assert selection(vals, det, 1, 1, None)[0][0] == (1, 5, ncols, 0)
            assert selection(vals, det, 1, 1, karr)[0][0][:2] == (5, 5) and karr[5] < karr[1]
            check_price(case, dev, mat, bvecs[:2], 2, 1, [g0, g1], combos)
            check_price(case, dev, mat, bvecs[:1], 1, 1, None, combos[:1])           # the empty column without g: X = 0
            # nside 2; the a side of problem 1 is zero: nothing is eligible there
            sides = [bvecs[0], bvecs[2], bvecs[1], [0] * n]
            got = f.price(dev, *slab([v for s in sides for v in s]), nprob=2, sides=2, cost=slab(g0 + g1), winners=True)
            assert (int(got[0][1]), int(got[1][1]), int(got[2][1]), int(got[3][1])) == (-1, 0, 0, 0)
            assert not got[4][2:].any()
            check_price(case, dev, mat, sides, 2, 2, [g0, g1], combos)
        finally:
            dev.close()


# ---- 3. width classes of slip_product_kernel: <= 64, 65-128, 129-192, 193-256 and > 256 digits ----

WIDTH_SHIFTS = (0, 70, 135, 200, 280)


def check_width_classes(lib_path, ncols, name="gen_n40", combos=COMBOS, sides=(2, 1), **kw):
    """five problems whose right-hand sides are multiplied by powers of 2^32 (y scales with them) so that the widths W of
    slip_product_kernel fall in each of its classes, asserted from the oracle before price is called.  With nside = 2 the widest
    problem has its x side = 3 * its a side: every eligible column ties, and the exact comparisons of the selection form
    products above 256 digits (the memory path there, asserted).  sides: the emulator runs nside = 1 alone."""
    with Case(lib_path, name, **kw) as case:
        n, det = case.n, case.det
        mat = Mat(n, ncols, shifted(n, case.cols, ncols))
        base = small_rhs(n, 10, 41)
        bvecs = []
        for c, s in enumerate(WIDTH_SHIFTS):
            a = [v * B ** s for v in base[2 * c + 1]]
            x = [3 * v for v in a] if s == WIDTH_SHIFTS[-1] else [v * B ** s for v in base[2 * c]]
            bvecs += [x, a]
        gs = small_costs(ncols, 5, 42)
        dev = mat.device(lib_path)
        try:
            for nside in sides:
                def every_class(vals, y):
                    classes = {min((w - 1) // 64, 4) for w in widths(mat, n, y, det, 5 * nside, nside, gs if nside == 1 else None)}
                    assert classes == {0, 1, 2, 3, 4}, sorted(classes)

                paths = check_price(case, dev, mat, bvecs[::3 - nside], 5, nside, gs if nside == 1 else None,
                                    combos if nside == 2 else combos[:1], plain=False, inspect=every_class)
                if nside == 2:
                    assert paths[3] > 0, "the memory path of the selection (cross products above 256 digits) was not reached"
        finally:
            dev.close()


def check_natural_wide(lib_path, name="de080285"):
    """a golden whose y is hundreds of limbs wide: one nside = 2 call with two problems"""
    with Case(lib_path, name) as case:
        n = case.n
        mat = Mat(n, 40, shifted(n, case.cols, 30) + random_columns(n, 10, 51))
        probs = handle_problems(n, case.cols, case.q, 52)[::2]
        bvecs = [side for pr in probs for side in pr]

        def wide(vals, y):
            assert max(widths(mat, n, y, case.det, 4, 2, None)) > 256

        dev = mat.device(lib_path)
        try:
            paths = check_price(case, dev, mat, bvecs, 2, 2, None, ((1, True),), plain=False, inspect=wide)
            assert paths[3] > 0
        finally:
            dev.close()


# ---- 4. goldens ----

def check_golden(lib_path, name, combos=COMBOS, light=False, negative=False, sides=(1, 2), **kw):
    """M: the shifted columns of A and ten random sparse small-integer columns; three problems (ratio_helpers.handle_problems),
    the last with its x side = 3 * its a side, where every eligible column ties (light, for the emulator: the first and the
    last problem, or with one nside the last alone; fewer shifted columns)"""
    with Case(lib_path, name, negative=negative, **kw) as case:
        n = case.n
        if negative:
            assert case.det < 0, "det must be negative on this handle"
        mat = Mat(n, (8 if light else n) + 10, shifted(n, case.cols, 8 if light else n) + random_columns(n, 10, 61))
        probs = handle_problems(n, case.cols, case.q, 62)
        if light:
            probs = probs[::2] if len(sides) > 1 else probs[2:]
        nprob = len(probs)
        gs = small_costs(mat.ncols, nprob, 63)
        dev = mat.device(lib_path)
        try:
            def all_tie(vals, y):                                    # in the last problem, under one sense or the other
                assert max(selection(vals, case.det, 2, s, None)[0][-1][1] for s in (1, -1)) > 1

            for nside in sides:
                bvecs = [side for pr in probs for side in pr[:nside]]
                check_price(case, dev, mat, bvecs, nprob, nside, gs if nside == 1 else None, combos, plain=not light,
                            inspect=all_tie if nside == 2 else None)
                if not light:
                    check_price(case, dev, mat, bvecs, nprob, nside, None if nside == 1 else gs, combos[1:3], plain=False)
        finally:
            dev.close()
        return case.det


# ---- 6. grouping ----

def check_groups(lib_path, monkeypatch, name="gen_n40", **kw):
    """a staging bound below one problem's need: every problem is its own group, the results are those of the ungrouped call"""
    with Case(lib_path, name, **kw) as case:
        n = case.n
        mat = Mat(n, 20, shifted(n, case.cols, 14) + random_columns(n, 6, 71))
        gs = small_costs(20, 3, 72)
        dev = mat.device(lib_path)
        try:
            for nside in (1, 2):
                bvecs = small_rhs(n, 3 * nside, 73)
                b, cost = slab([v for bb in bvecs for v in bb]), slab([v for g in gs for v in g])
                whole = case.f.price(dev, *b, nprob=3, sides=nside, cost=cost, sense=-1, winners=True)
                monkeypatch.setenv("SLIP_HIP_PRODUCT_STAGE_KB", "1")
                parts = case.f.price(dev, *b, nprob=3, sides=nside, cost=cost, sense=-1, winners=True)
                assert all(np.array_equal(u, v) for u, v in zip(whole, parts))
                check_price(case, dev, mat, bvecs, 3, nside, gs, ((-1, True),), plain=False)
                monkeypatch.delenv("SLIP_HIP_PRODUCT_STAGE_KB")
        finally:
            dev.close()


# ---- 7. lifecycle ----

def check_lifecycle(lib_path, name="gen_n40", **kw):
    import slip_lu_amd as sl
    with Case(lib_path, name, **kw) as case:
        n, f, q = case.n, case.f, case.q
        mat = Mat(n, 12, shifted(n, case.cols, 8) + random_columns(n, 4, 81))
        bvecs = small_rhs(n, 2, 82)
        b, rhs = slab([v for bb in bvecs for v in bb]), slab(bvecs[0])
        gs = small_costs(12, 1, 83)
        cost = slab(gs[0])
        yv = slab([(-1) ** t * (t + 2 ** (5 * t)) for t in range(n)])
        dev = mat.device(lib_path)
        try:
            x0, t0, m0 = f.solve(*rhs), f.solve_transpose(*rhs), dev.multiply(*yv, transpose=True)
            first = f.price(dev, *b, sides=2, cost=cost, winners=True)
            again = f.price(dev, *b, sides=2, cost=cost, winners=True)                # twice in a row: identical
            assert all(np.array_equal(u, v) for u, v in zip(first, again))
            for before, after in ((x0, f.solve(*rhs)), (t0, f.solve_transpose(*rhs)), (m0, dev.multiply(*yv, transpose=True))):
                assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
            check_price(case, dev, mat, bvecs, 1, 2, gs, ((1, False),), plain=False)
            # a handle around a download of the same factors: the same answers
            g = sl.Factorization.from_factors(f.download(), lib_path=lib_path, **{k: v for k, v in kw.items() if k in ("waves", "workers")})
            try:
                given = g.price(dev, *b, sides=2, cost=cost, winners=True)
                assert all(np.array_equal(u, v) for u, v in zip(first, given))
                given = g.price(dev, *rhs, sides=1, sense=-1, winners=True)
                assert all(np.array_equal(u, v) for u, v in zip(f.price(dev, *rhs, sides=1, sense=-1, winners=True), given))
            finally:
                g.close()
            # a column replaced and factorised again: the answer for the NEW matrix, as a fresh handle gives it
            cols = [dict(c) for c in case.cols]
            j = int(q[n // 2])
            new = dict(cols[int(q[n - 1])])
            new[j % n] = new.get(j % n, 0) + 2 ** 40 + 1
            f.replace_column(j, list(new), list(new.values()))
            f.run(0)
            cols[j] = new
            replaced = f.price(dev, *b, sides=2, cost=cost, winners=True)
            nAp = np.cumsum([0] + [len(c) for c in cols]).astype(np.int64)
            nAi = np.array([r for c in cols for r in c], np.int32)
            nAlen, nAlimbs = slab([v for c in cols for v in c.values()])
            h = sl.Factorization(n, nAp, nAi, nAlen, nAlimbs, q, lib_path=lib_path, **kw)
            try:
                h.run(0)
                fresh = h.price(dev, *b, sides=2, cost=cost, winners=True)
                assert all(np.array_equal(u, v) for u, v in zip(replaced, fresh))
            finally:
                h.close()
            case.det = oracle_lib.bigints(*f.pivots())[-1]
            check_price(case, dev, mat, bvecs, 1, 2, gs, ((-1, True),), plain=False)
            m1 = dev.multiply(*yv, transpose=True)
            assert np.array_equal(m0[0], m1[0]) and np.array_equal(m0[1], m1[1])
        finally:
            dev.close()


# ---- 8. rejections: SLIP_HIP_INCORRECT_INPUT (-3), nothing written ----

def check_rejections(lib_path, name="gen_n40", **kw):
    import slip_lu_amd as sl
    from slip_lu_amd import _lib
    lib = _lib.load(lib_path)
    _, fix = load_case(name)
    n, Ap, Ai, Alen, Alimbs, q = len(fix["q"]), fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"]
    cols = columns(n, Ap, Ai, oracle_lib.bigints(Alen, Alimbs))
    mat = Mat(n, 5, shifted(n, cols, 5))
    other = Mat(n + 1, 5, shifted(n, cols, 5))
    b = slab([(-1) ** t * (t % 7) for t in range(2 * n)])
    glen, glimbs = slab([3, -(2 ** 64), 0, 1, 2 ** 70])
    res = [np.full(2, 77, np.int32) for _ in range(4)]
    R = [r.ctypes.data for r in res]
    bl, bv, G = b[0].ctypes.data, b[1].ctypes.data, (glen.ctypes.data, glimbs.ctypes.data, glimbs.size)
    NOG = (None, None, 0)
    pl, px, nl = C.c_void_p(), C.c_void_p(), C.c_int64()
    outs, none = (C.byref(pl), C.byref(px), C.byref(nl)), (None, None, None)
    f = sl.Factorization(n, Ap, Ai, Alen, Alimbs, q, lib_path=lib_path, **kw)
    dev, wrong = mat.device(lib_path), other.device(lib_path)
    fn = lib.slip_hip_factor_price
    try:
        f.run(n // 2)
        assert f.info()["K"] < n
        assert fn(f.h, dev.h, 1, 1, bl, bv, *G, 1, None, *R, *outs, None) == -3          # a run to K < n
        with pytest.raises(sl.SlipError) as e:
            f.price(dev, *b, sides=2)
        assert e.value.code == -3
        f.run(0)
        bad = [(None, dev.h, 1, 1, bl, bv, *G, 1, None, *R, *outs, None), (f.h, None, 1, 1, bl, bv, *G, 1, None, *R, *outs, None),
               (f.h, dev.h, 1, 1, None, bv, *G, 1, None, *R, *outs, None), (f.h, dev.h, 1, 1, bl, None, *G, 1, None, *R, *outs, None),
               (f.h, wrong.h, 1, 1, bl, bv, *NOG, 1, None, *R, *outs, None),                                    # M->m != n
               (f.h, dev.h, 0, 1, bl, bv, *G, 1, None, *R, *outs, None), (f.h, dev.h, 3, 1, bl, bv, *G, 1, None, *R, *outs, None),
               (f.h, dev.h, 2, 0, bl, bv, *G, 1, None, *R, *outs, None), (f.h, dev.h, 1, -1, bl, bv, *G, 1, None, *R, *outs, None),
               (f.h, dev.h, 1, 1, bl, bv, *G, 0, None, *R, *outs, None), (f.h, dev.h, 1, 1, bl, bv, *G, 2, None, *R, *outs, None),
               (f.h, dev.h, 1, 1, bl, bv, None, G[1], G[2], 1, None, *R, *outs, None),                         # one of glen / glimbs
               (f.h, dev.h, 1, 1, bl, bv, G[0], None, G[2], 1, None, *R, *outs, None),
               (f.h, dev.h, 1, 1, bl, bv, G[0], G[1], G[2] - 1, 1, None, *R, *outs, None),                     # g longer than g_limbs
               (f.h, dev.h, 1, 1, bl, bv, *G, 1, None, *R, outs[0], None, outs[2], None),                      # partial winners' triples
               (f.h, dev.h, 1, 1, bl, bv, *G, 1, None, *R, None, outs[1], outs[2], None),
               (f.h, dev.h, 1, 1, bl, bv, *G, 1, None, *R, outs[0], outs[1], None, None),
               (f.h, dev.h, 1, 1, bl, bv, *G, 1, None, *R, None, None, outs[2], None)]
        bad += [(f.h, dev.h, 1, 1, bl, bv, *G, 1, None, *[None if t == k else r for t, r in enumerate(R)], *outs, None) for k in range(4)]
        for args in bad:
            assert fn(*args) == -3, args[2:4]
        assert all((r == 77).all() for r in res) and pl.value is None and px.value is None and nl.value == 0
        assert lib.slip_hip_factor_price_ms(f.h, None) == -3 and lib.slip_hip_factor_price_ms(None, R[0]) == -3
        assert lib.slip_hip_factor_price_paths(f.h, None) == -3 and lib.slip_hip_factor_price_paths(None, R[0]) == -3
        with pytest.raises(ValueError):
            f.price(dev, *b, nprob=3, sides=1)
        with pytest.raises(ValueError):
            f.price(dev, *b, sides=2, key=np.zeros(6, np.int32))
        with pytest.raises(ValueError):
            f.price(dev, *b, sides=2, cost=slab([1, 2, 3]))
        # the same arguments, accepted
        assert fn(f.h, dev.h, 1, 1, bl, bv, *G, 1, None, *R, *none, None) == 0
        assert all(r[0] != 77 and r[1] == 77 for r in res)
    finally:
        f.close()
        dev.close()
        wrong.close()
