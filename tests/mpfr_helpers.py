"""Shared by tests/test_emu_mpfr.py (the emulator build) and tests/test_gpu_mpfr.py (the product on the device): the conversion of
exact solutions to multi-precision floats (slip_hip_solution_to_mpfr, slip_hip_factor_solve_mpfr) against round_mpfr, a model in
Python integers of what MPFR's mpfr_set_q leaves, and against MPFR's own answers recorded in
tests/golden/mpfr_corpus.json.gz.  Every comparison is of sign, exponent, every limb of the mantissa and the ternary value.
lib_path None is the product library."""
import gzip
import json
import os

import numpy as np
import pytest

import oracle_lib
import slabfile
from check_helpers import slab
from conftest import GOLDEN, load_case, solve_inputs
from todouble_helpers import SOLVE_CASES, TSOLVE_CASES, handle, integer_rhs, padded_slab, rhs_pattern

RNDN, RNDZ, RNDU, RNDD, RNDA = range(5)
MODES = (RNDN, RNDZ, RNDU, RNDD, RNDA)


def round_mpfr(N, D, prec, rnd):
    """N / D (D != 0) rounded to prec bits as mpfr_set_q does: (sign, exp, m, ternary) with |x| = m * 2^(exp - prec),
    2^(prec-1) <= m < 2^prec; a zero is (0, 0, 0, 0) -- always +0; ternary is the sign of (rounded - exact)"""
    if D == 0:
        raise ZeroDivisionError("round_mpfr: zero denominator")
    if not 2 <= prec <= 65536 or rnd not in MODES:
        raise ValueError("round_mpfr: prec or rnd")
    if N == 0:
        return 0, 0, 0, 0
    neg = (N < 0) != (D < 0)
    n, d = abs(N), abs(D)
    e0 = n.bit_length() - d.bit_length()                    # 2^(e0-1) <= n / d < 2^e0 for this e0 or the next
    if (n << max(-e0, 0)) >= (d << max(e0, 0)):
        e0 += 1
    s = prec + 1 - e0                                       # t = floor(n / d * 2^s) has prec + 1 bits
    t, r = divmod(n << s, d) if s >= 0 else divmod(n, d << -s)
    assert t.bit_length() == prec + 1
    m0, rb, st = t >> 1, t & 1, int(r != 0)
    if rnd == RNDN:
        inc = rb & (st | (m0 & 1))
    else:
        away = rnd == RNDA or (rnd == RNDU and not neg) or (rnd == RNDD and neg)
        inc = (rb | st) if away else 0
    m, e = m0 + inc, e0
    if m >> prec:
        m, e = 1 << (prec - 1), e0 + 1
    tern = 0 if not (rb | st) else (1 if bool(inc) != neg else -1)
    return (-1 if neg else 1), e, m, tern


def limbs_of(m, prec):
    """the mantissa m left-aligned in ceil(prec / 64) limbs, least significant first (MPFR's limb image)"""
    nl = (prec + 63) // 64
    image = m << (64 * nl - prec)
    return [(image >> (64 * k)) & (2 ** 64 - 1) for k in range(nl)]


def assert_same_mpfr(got, want, prec, what):
    """got: (sign, exp, mant, ternary) arrays of a call; want: one round_mpfr tuple per entry"""
    sign, exp, mant, tern = got
    assert len(sign) == len(exp) == len(mant) == len(tern) == len(want), (what, len(sign), len(want))
    assert mant.shape == (len(want), (prec + 63) // 64) and mant.dtype == np.uint64, (what, mant.shape)
    bad = []
    for t, (s, e, m, tv) in enumerate(want):
        have = (int(sign[t]), int(exp[t]), [int(v) for v in mant[t]], int(tern[t]))
        if have != (s, e, limbs_of(m, prec), tv):
            bad.append((t, have[0], have[1], have[3], s, e, tv, hex(sum(v << (64 * k) for k, v in enumerate(have[2])) >> (64 * len(have[2]) - prec)), hex(m)))
    assert not bad, (what, len(bad), bad[:4])


def load_corpus():
    """the corpus with its numbers as Python ints: dict(den, prec, prec_den, pad, rows, res) -- rows[c][pi] the numerators of
    denominator c at precision index pi (generic ones first), pad[pi] the high zero limbs each gets in a slab,
    res[c][pi][t][rnd] = MPFR's (sign, exp, m, ternary)"""
    doc = json.loads(gzip.open(os.path.join(GOLDEN, "mpfr_corpus.json.gz")).read())
    den = [int(v, 16) for v in doc["den"]]
    value = lambda c, e: e[0] * (int(e[1], 16) * abs(den[c]) + int(e[2], 16))      # noqa: E731
    rows, res = [], []
    for c in range(len(den)):
        g = [value(c, e) for e in doc["num"][c]]
        rows.append([[g[t] for t in doc["gsel"][pi]] + [value(c, e) for e in doc["pnum"][c][pi]] if c in doc["prec_den"][pi] else []
                     for pi in range(len(doc["prec"]))])
        res.append([[[(sg, e, int(ent["m"][k], 16) if sg else 0, t) for sg, e, k, t in ent["v"]] for ent in per] for per in doc["res"][c]])
    return dict(den=den, prec=doc["prec"], prec_den=doc["prec_den"], pad=doc["pad"], rows=rows, res=res,
                generic=doc["generic"], shapes=doc["shapes"])


def check_corpus(lib_path, precs=None):
    """every (precision, mode) of the corpus as ONE call, n = numerators per denominator, nrhs = the denominators recorded for
    that precision: every entry equals MPFR's.  Returns (entries compared, the path counts summed over the calls)."""
    import slip_lu_amd as sl
    co = load_corpus()
    total, paths = 0, [0, 0, 0, 0]
    for pi, p in enumerate(co["prec"]):
        if precs is not None and p not in precs:
            continue
        keep = co["prec_den"][pi]
        n = len(co["pad"][pi])
        xlen, xlimbs = padded_slab([N for c in keep for N in co["rows"][c][pi]], [q for c in keep for q in co["pad"][pi]])
        dlen, dlimbs = padded_slab([co["den"][c] for c in keep], [c % 2 for c in keep])      # every other one with a high zero limb
        for rnd in MODES:
            got = sl.solution_to_mpfr(n, xlen, xlimbs, dlen, dlimbs, nrhs=len(keep), prec=p, rnd=rnd, lib_path=lib_path)
            assert_same_mpfr(got, [co["res"][c][pi][t][rnd] for c in keep for t in range(n)], p, ("corpus", p, rnd))
            paths = [a + b for a, b in zip(paths, sl.solution_to_mpfr_paths(lib_path=lib_path))]
            total += n * len(keep)
    return total, paths


def expected(nums, den, prec, rnd, order=None):
    """round_mpfr of nums[p] / den placed at order[p] (None: at p)"""
    want = [None] * len(nums)
    for p, v in enumerate(nums):
        want[int(order[p]) if order is not None else p] = round_mpfr(v, den, prec, rnd)
    return want


def check_reference_solutions(lib_path, name, nrhs=3, precs=(53, 128), **kw):
    """solve_mpfr of solve_rhs(n) == round_mpfr of the reference's own rationals (tests/golden/solve_*), placed at q[p]; every
    right-hand side == round_mpfr of the same handle's `solve` numerators over det; all five modes"""
    n, Ap, Ai, Alen, Alimbs, q, fix = solve_inputs(SOLVE_CASES[name])
    num = oracle_lib.bigints(fix["xnumlen"], fix["xnumlimbs"])
    den = oracle_lib.bigints(fix["xdenlen"], fix["xdenlimbs"])
    bs = rhs_pattern(oracle_lib.solve_rhs(n), nrhs)
    blen, blimbs = slab([v for b in bs for v in b])
    f, det = handle(lib_path, n, Ap, Ai, Alen, Alimbs, q, **kw)
    try:
        x = oracle_lib.bigints(*f.solve(blen, blimbs, nrhs=nrhs))
        for prec in precs:
            for rnd in MODES:
                got = f.solve_mpfr(blen, blimbs, nrhs=nrhs, prec=prec, rnd=rnd)
                assert f.to_mpfr_ms() >= 0 and sum(f.to_mpfr_paths()) == n * nrhs
                ref = [None] * n
                for p in range(n):
                    ref[int(q[p])] = round_mpfr(num[p], den[p], prec, rnd)
                assert_same_mpfr(tuple(a[:n] for a in got), ref, prec, (name, prec, rnd, "reference"))
                want = [w for c in range(nrhs) for w in expected(x[c * n:(c + 1) * n], det, prec, rnd, q)]
                assert_same_mpfr(got, want, prec, (name, prec, rnd))
    finally:
        f.close()


def check_reference_tsolutions(lib_path, name, nrhs=3, precs=(53, 128), **kw):
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
        x = oracle_lib.bigints(*f.solve_transpose(blen, blimbs, nrhs=nrhs))
        for prec in precs:
            for rnd in MODES:
                got = f.solve_mpfr(blen, blimbs, nrhs=nrhs, transpose=True, prec=prec, rnd=rnd)
                ref = [None] * n
                for p in range(n):
                    ref[int(fix["q"][p])] = round_mpfr(num[p], den[p], prec, rnd)
                assert_same_mpfr(tuple(a[:n] for a in got), ref, prec, (name, prec, rnd, "reference"))
                want = [w for c in range(nrhs) for w in expected(x[c * n:(c + 1) * n], det, prec, rnd)]
                assert_same_mpfr(got, want, prec, (name, "T", prec, rnd))
    finally:
        f.close()


def check_integer_solutions(lib_path, name, prec=64, **kw):
    """b = A(:,q) x0 with small integer x0 (a third of it zero, two filling the precision): every mode returns x0 itself with
    ternary 0 -- the quotient is exact, the remainder of the long division must come out as zero"""
    n, Ap, Ai, Alen, Alimbs, q, _ = solve_inputs(SOLVE_CASES[name])
    x0 = [0 if p % 3 == 0 else ((p * 7919) % 41) - 20 for p in range(n)]
    x0[1], x0[2] = 2 ** prec - 1, -(2 ** (prec - 1) + 1)
    blen, blimbs = slab(integer_rhs(n, Ap, Ai, Alen, Alimbs, q, x0))
    f, det = handle(lib_path, n, Ap, Ai, Alen, Alimbs, q, **kw)
    try:
        got = [f.solve_mpfr(blen, blimbs, prec=prec, rnd=rnd) for rnd in MODES]
        paths = f.to_mpfr_paths()
    finally:
        f.close()
    want = expected(x0, 1, prec, RNDZ, q)
    assert all(w[3] == 0 for w in want)
    for rnd in MODES:
        assert not got[rnd][3].any(), (name, rnd, "ternary")
        assert_same_mpfr(got[rnd], want, prec, (name, rnd))
    assert paths[3] == sum(v == 0 for v in x0)
    return paths


SCALES = [(3000, 7), (-3000, 7), (3000, -7)]                # 1000 / (7/3), and with a negative part


def check_scale(lib_path, name, prec=128, **kw):
    """scale = snum / sden applied before the ONE rounding: round_mpfr(xnum * snum, det * sden), plain and transposed, all modes
    (a negative scale turns RNDU into rounding the magnitude down); zeros stay +0; a zero scale part is
    SLIP_HIP_INCORRECT_INPUT"""
    import slip_lu_amd as sl
    n, Ap, Ai, Alen, Alimbs, q, _ = solve_inputs(SOLVE_CASES[name])
    bs = rhs_pattern(oracle_lib.solve_rhs(n), 2)
    blen, blimbs = slab([v for b in bs for v in b])
    f, det = handle(lib_path, n, Ap, Ai, Alen, Alimbs, q, **kw)
    try:
        x = oracle_lib.bigints(*f.solve(blen, blimbs, nrhs=2))
        xt = oracle_lib.bigints(*f.solve_transpose(blen, blimbs, nrhs=2))
        for sn, sd in SCALES:
            for rnd in MODES:
                got = f.solve_mpfr(blen, blimbs, nrhs=2, scale=(sn, sd), prec=prec, rnd=rnd)
                want = [w for c in range(2) for w in expected([v * sn for v in x[c * n:(c + 1) * n]], det * sd, prec, rnd, q)]
                assert_same_mpfr(got, want, prec, (name, sn, sd, rnd))
                got = f.solve_mpfr(blen, blimbs, nrhs=2, transpose=True, scale=(sn, sd), prec=prec, rnd=rnd)
                want = [w for c in range(2) for w in expected([v * sn for v in xt[c * n:(c + 1) * n]], det * sd, prec, rnd)]
                assert_same_mpfr(got, want, prec, (name, "T", sn, sd, rnd))
        for bad in ((0, 1), (1, 0), (0, 0)):
            with pytest.raises(sl.SlipError) as e:
                f.solve_mpfr(blen, blimbs, nrhs=2, scale=bad)
            assert e.value.code == -3
    finally:
        f.close()


def check_lifecycle(lib_path, name="solve_test_mat", **kw):
    """refused before the factorisation is complete and for nrhs < 1; `solve`, `solve_double` and `solve_rational` return what
    they did before a solve_mpfr; the same floats after reset + run; on a handle around given factors the plain call is refused
    and the transposed one works"""
    import slip_lu_amd as sl
    n, Ap, Ai, Alen, Alimbs, q, _ = solve_inputs(SOLVE_CASES[name])
    b = [int(v) for v in oracle_lib.solve_rhs(n)]
    blen, blimbs = slab(b)
    same = lambda a, c: all(np.array_equal(u, v) for u, v in zip(a, c))      # noqa: E731
    f = sl.Factorization(n, Ap, Ai, Alen, Alimbs, q, lib_path=lib_path, **kw)
    try:
        f.run(n // 2)
        for tr in (False, True):
            with pytest.raises(sl.SlipError) as e:
                f.solve_mpfr(blen, blimbs, transpose=tr)
            assert e.value.code == -3
        f.run(0)
        with pytest.raises(sl.SlipError) as e:
            f.solve_mpfr(blen[:0], blimbs, nrhs=0)
        assert e.value.code == -3
        det = oracle_lib.bigints(*f.pivots())[-1]
        x0, d0, r0 = f.solve(blen, blimbs), f.solve_double(blen, blimbs), f.solve_rational(blen, blimbs)
        m0 = f.solve_mpfr(blen, blimbs, prec=200, rnd=RNDN)
        t0 = f.solve_mpfr(blen, blimbs, transpose=True, prec=200, rnd=RNDD)
        assert_same_mpfr(m0, expected(oracle_lib.bigints(*x0), det, 200, RNDN, q), 200, "first")
        assert same(f.solve(blen, blimbs), x0) and same([f.solve_double(blen, blimbs)], [d0]) and same(f.solve_rational(blen, blimbs), r0)
        fac = f.download()
        f.reset()
        with pytest.raises(sl.SlipError):
            f.solve_mpfr(blen, blimbs)
        f.run(0)
        assert same(f.solve_mpfr(blen, blimbs, prec=200, rnd=RNDN), m0)
        assert same(f.solve_mpfr(blen, blimbs, transpose=True, prec=200, rnd=RNDD), t0)
        assert same(f.solve(blen, blimbs), x0) and same([f.solve_double(blen, blimbs)], [d0]) and same(f.solve_rational(blen, blimbs), r0)
    finally:
        f.close()
    g = sl.Factorization.from_factors(fac, lib_path=lib_path, **{k: v for k, v in kw.items() if k in ("waves", "workers")})
    try:
        with pytest.raises(sl.SlipError) as e:
            g.solve_mpfr(blen, blimbs)
        assert e.value.code == -3
        assert same(g.solve_mpfr(blen, blimbs, transpose=True, prec=200, rnd=RNDD), t0)
    finally:
        g.close()


def check_rejections(lib_path, name="solve_test_mat", **kw):
    """prec 1 and 65537, rnd 5 (MPFR_RNDF) and -1 (MPFR_RNDNA), on both entry points; slip_hip_solution_to_mpfr: nrhs < 1, a zero
    denominator, a limb array longer than its capacity, a missing output"""
    import slip_lu_amd as sl
    from slip_lu_amd import _lib
    lib = _lib.load(lib_path)
    xlen, xlimbs = slab([5, -7, 2 ** 64])
    dlen, dlimbs = slab([3])
    assert_same_mpfr(sl.solution_to_mpfr(3, xlen, xlimbs, dlen, dlimbs, prec=10, rnd=RNDU, lib_path=lib_path),
                     [round_mpfr(v, 3, 10, RNDU) for v in (5, -7, 2 ** 64)], 10, "small")
    assert round_mpfr(7, 2, 2, RNDN) == (1, 3, 2, 1) and round_mpfr(2 ** 64 - 1, 1, 10, RNDN)[1] == 65
    for prec, rnd in ((1, 0), (65537, 0), (0, 0), (-5, 0), (53, 5), (53, -1), (53, 17)):
        with pytest.raises(sl.SlipError) as e:
            sl.solution_to_mpfr(3, xlen, xlimbs, dlen, dlimbs, prec=prec, rnd=rnd, lib_path=lib_path)
        assert e.value.code == -3, (prec, rnd)
    sign, exp, mant, tern = np.zeros(3, np.int8), np.zeros(3, np.int64), np.zeros(3, np.uint64), np.zeros(3, np.int8)
    call = lambda n, nrhs, xcap, dl, dv, dcap, so=sign: lib.slip_hip_solution_to_mpfr(      # noqa: E731
        n, nrhs, xlen.ctypes.data, xlimbs.ctypes.data, xcap, dl.ctypes.data, dv.ctypes.data, dcap, 53, 0,
        so.ctypes.data if so is not None else None, exp.ctypes.data, mant.ctypes.data, tern.ctypes.data, None)
    assert call(3, 1, xlimbs.size, dlen, dlimbs, 1) == 0
    assert call(3, 0, xlimbs.size, dlen, dlimbs, 1) == -3
    assert call(3, 1, xlimbs.size - 1, dlen, dlimbs, 1) == -3                     # a short slab
    assert call(3, 1, xlimbs.size, dlen, dlimbs, 0) == -3
    assert call(3, 1, xlimbs.size, np.zeros(1, np.int32), dlimbs, 1) == -3        # d = 0: no limbs
    assert call(3, 1, xlimbs.size, np.array([1], np.int32), np.zeros(1, np.uint64), 1) == -3      # d = 0: one limb that is zero
    assert call(3, 1, xlimbs.size, dlen, dlimbs, 1, None) == -3
    assert lib.slip_hip_solution_to_mpfr(3, 1, xlen.ctypes.data, xlimbs.ctypes.data, xlimbs.size, dlen.ctypes.data, dlimbs.ctypes.data, 1,
                                         53, 0, sign.ctypes.data, exp.ctypes.data, mant.ctypes.data, None, None) == 0      # no ternary wanted
    n, Ap, Ai, Alen, Alimbs, q, _ = solve_inputs(SOLVE_CASES[name])
    blen, blimbs = slab([int(v) for v in oracle_lib.solve_rhs(n)])
    f, _ = handle(lib_path, n, Ap, Ai, Alen, Alimbs, q, **kw)
    try:
        for prec, rnd in ((1, 0), (65537, 0), (53, 5), (53, -1)):
            with pytest.raises(sl.SlipError) as e:
                f.solve_mpfr(blen, blimbs, prec=prec, rnd=rnd)
            assert e.value.code == -3, (prec, rnd)
        f.solve_mpfr(blen, blimbs, prec=2, rnd=4)
    finally:
        f.close()


def check_wide_handle(lib_path, name, prec=128):
    """a complete factorisation whose determinant exceeds 256 digits: solve_mpfr == round_mpfr of the same handle's `solve`
    numerators over det, entry by entry, nearest and away; an integer solution comes back exactly; the wide path is counted"""
    entry, fix = load_case(name)
    n, q = len(fix["q"]), fix["q"]
    f, det = handle(lib_path, n, fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], q, pivot=entry["pivot"], tol=entry["tol"])
    try:
        assert det.bit_length() > 256 * 32
        b = [int(v) for v in oracle_lib.solve_rhs(n)]
        x0 = [((p * 31) % 7) - 3 for p in range(n)]
        bi = integer_rhs(n, fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], q, x0)
        blen, blimbs = slab(b + bi)
        x = oracle_lib.bigints(*f.solve(blen, blimbs, nrhs=2))
        for rnd in (RNDN, RNDA):
            got = f.solve_mpfr(blen, blimbs, nrhs=2, prec=prec, rnd=rnd)
            paths = f.to_mpfr_paths()
            want = [w for c in range(2) for w in expected(x[c * n:(c + 1) * n], det, prec, rnd, q)]
            assert_same_mpfr(got, want, prec, (name, rnd))
            assert_same_mpfr(tuple(a[n:] for a in got), expected(x0, 1, prec, rnd, q), prec, (name, rnd, "integers"))
            assert paths[2] > 0 and paths[1] == 0 and sum(paths) == 2 * n
    finally:
        f.close()
