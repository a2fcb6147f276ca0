"""Shared by tests/test_emu_bound.py (the emulator build) and tests/test_gpu_bound.py (the product on the device): bounds in the
exact selections (slip_hip_ratio_test_bounded, slip_hip_bound_test on caller slabs; slip_hip_factor_ratio_test_bounded,
slip_hip_factor_bound_test fused with a solve on a handle).  The oracle is Python, in the DIRECT formulation on the true values
x = xnum / d, alpha = anum / d, l = lo / den, u = hi / den: the step (x - l) / t resp. (x - u) / t with t = sense * alpha, and the
largest true violation max(l - x, x - u); every comparison is exact equality, of all results and of the winners' slab.
lib_path None is the product library."""
import ctypes as C
import random
from fractions import Fraction

import numpy as np
import pytest

import oracle_lib
from check_helpers import columns, slab
from conftest import load_case
from product_helpers import BORDER_W, same_slab
from ratio_helpers import handle_problems, padded_slab

B = 2 ** 32
TOP = B - 1


def digits(v):
    return (abs(v).bit_length() + 31) // 32


# ---- the oracle ----

def oracle_steps(xs, avs, d, bnd, sense):
    """{i: (step, side)} of the eligible entries of one problem"""
    el = {}
    for i, (x, a) in enumerate(zip(xs, avs)):
        t, k = sense * Fraction(a, d), bnd["kind"][i]
        if t > 0 and k & 1:
            el[i] = ((Fraction(x, d) - Fraction(bnd["lo"][i], bnd["den"])) / t, -1)
        elif t < 0 and k & 2:
            el[i] = ((Fraction(x, d) - Fraction(bnd["hi"][i], bnd["den"])) / t, 1)
    return el


def oracle_violations(xs, d, bnd):
    """{i: (violation, side)} of the violated entries of one vector"""
    out = {}
    for i, x in enumerate(xs):
        k, xv = bnd["kind"][i], Fraction(x, d)
        vlo = Fraction(bnd["lo"][i], bnd["den"]) - xv if k & 1 else 0
        vhi = xv - Fraction(bnd["hi"][i], bnd["den"]) if k & 2 else 0
        if max(vlo, vhi) > 0:
            out[i] = (max(vlo, vhi), -1 if vlo >= vhi else 1)
    return out


def pick(el, key, largest=False):
    """((best, nties, count, side), ties): the extreme value, among ties the smallest (key, i)"""
    if not el:
        return (-1, 0, 0, 0), []
    m = (max if largest else min)(v for v, _ in el.values())
    ties = [i for i in el if el[i][0] == m]
    best = min(ties, key=lambda i: (int(key[i]) if key is not None else 0, i))
    return (best, len(ties), len(el), el[best][1]), ties


def winner_ratio(xs, avs, d, bnd, best, side):
    """(N_best, a'_best) by the definition of the header"""
    if best < 0:
        return 0, 0
    if side < 0:
        return bnd["den"] * xs[best] - d * bnd["lo"][best], avs[best]
    return d * bnd["hi"][best] - bnd["den"] * xs[best], -avs[best]


def winner_violation(el, d, bnd, best):
    """v_worst as an integer over |d| * den"""
    v = el[best][0] * abs(d) * bnd["den"] if best >= 0 else 0
    assert v.denominator == 1 if best >= 0 else True
    return int(v)


# ---- calls ----

def make_bounds(n, bnd, pad=None):
    """an sl.Bounds of the dictionary kind / lo / hi / den; a side no entry switches on is not passed; pad: high zero limbs on
    every entry of lo and hi (t % 3 of them) and two on den"""
    import slip_lu_amd as sl
    need = [any(k & bit for k in bnd["kind"]) for bit in (1, 2)]
    pads = [t % 3 for t in range(n)] if pad else None
    lo = padded_slab(bnd["lo"], pads) if need[0] else None
    hi = padded_slab(bnd["hi"], pads) if need[1] else None
    b = sl.Bounds(n, np.array(bnd["kind"], np.int32), lo, hi, bnd["den"])
    if pad:
        dl, dv = padded_slab([bnd["den"]], [2])
        b.padded_den = (dl, dv)
        b.rec.bdlen, b.rec.bdlimbs = int(dl[0]), dv.ctypes.data
    return b


def run_ratio(lib_path, probs, bnd, sense=1, key=None, pad=False):
    """one call of slip_hip_ratio_test_bounded on [(xs, avs, d), ...] against the oracle; returns (path counts, results, ties)"""
    import slip_lu_amd as sl
    n, nprob = len(probs[0][0]), len(probs)
    pads = [t % 3 for t in range(n * nprob)] if pad else None
    x = padded_slab([v for p in probs for v in p[0]], pads)
    a = padded_slab([v for p in probs for v in p[1]], pads)
    d = padded_slab([p[2] for p in probs], [1 + c % 2 for c in range(nprob)] if pad else None)
    got = sl.ratio_test_bounded(n, *x, *a, *d, make_bounds(n, bnd, pad), nprob=nprob, sense=sense, key=key, winners=True, lib_path=lib_path)
    want = [pick(oracle_steps(xs, avs, dd, bnd, sense), key) for xs, avs, dd in probs]
    for t, what in enumerate(("best", "nties", "neligible", "side")):
        assert [int(v) for v in got[t]] == [w[0][t] for w in want], (what, sense, key)
    same_slab(got[4:], [v for (xs, avs, dd), w in zip(probs, want) for v in winner_ratio(xs, avs, dd, bnd, w[0][0], w[0][3])],
              "the winners' N and a'")
    plain = sl.ratio_test_bounded(n, *x, *a, *d, make_bounds(n, bnd, pad), nprob=nprob, sense=sense, key=key, lib_path=lib_path)
    assert len(plain) == 4 and all(np.array_equal(u, v) for u, v in zip(plain, got[:4]))
    return sl.bound_paths(lib_path=lib_path), [w[0] for w in want], [w[1] for w in want]


def run_bound(lib_path, vecs, bnd, key=None, pad=False):
    """one call of slip_hip_bound_test on [(xs, d), ...] against the oracle; returns (path counts, results, ties)"""
    import slip_lu_amd as sl
    n, nprob = len(vecs[0][0]), len(vecs)
    pads = [t % 3 for t in range(n * nprob)] if pad else None
    x = padded_slab([v for p in vecs for v in p[0]], pads)
    d = padded_slab([p[1] for p in vecs], [1 + c % 2 for c in range(nprob)] if pad else None)
    got = sl.bound_test(n, *x, *d, make_bounds(n, bnd, pad), nprob=nprob, key=key, winners=True, lib_path=lib_path)
    els = [oracle_violations(xs, dd, bnd) for xs, dd in vecs]
    want = [pick(el, key, largest=True) for el in els]
    for t, what in enumerate(("worst", "nties", "nviolated", "side")):
        assert [int(v) for v in got[t]] == [w[0][t] for w in want], (what, key)
    same_slab(got[4:], [winner_violation(el, dd, bnd, w[0][0]) for el, (_, dd), w in zip(els, vecs, want)], "the worst violations")
    return sl.bound_paths(lib_path=lib_path), [w[0] for w in want], [w[1] for w in want]


# ---- 1. reduction to the existing ratio test: kind = 1, lo = 0, den = 1 (and 7: the denominator cancels) ----

SIGNS_X = [5, -7, 2 ** 200 + 3, -(2 ** 200 + 3), 0, 9, 0, -3, 11, 4, -4, 0]
SIGNS_A = [3, 2, -5, -(2 ** 200 + 3), 7, 0, 0, -1, 2 ** 70, -6, 6, -2 ** 64]        # ratio_helpers.check_signs_and_zeros's vectors


def check_reduction(lib_path):
    import slip_lu_amd as sl
    n = len(SIGNS_X)
    probs = [(SIGNS_X, SIGNS_A, 1), ([4, 1, 9] * 4, [2, 1, 3] * 4, 1), ([1, 2, 3] * 4, [-1, 0, -5] * 4, 1)]
    x, a = slab([v for p in probs for v in p[0]]), slab([v for p in probs for v in p[1]])
    for den in (1, 7):
        bnd = dict(kind=[1] * n, lo=[0] * n, hi=[0] * n, den=den)
        for sense in (1, -1):
            for key in (None, np.arange(n, dtype=np.int32)[::-1].copy()):
                paths, res, _ = run_ratio(lib_path, probs, bnd, sense, key)
                old = sl.ratio_test(n, *x, *a, nprob=len(probs), sense=sense, key=key, lib_path=lib_path)
                assert [r[:3] for r in res] == [tuple(int(o[c]) for o in old) for c in range(len(probs))], (den, sense)
                assert all(r[3] == (-1 if r[0] >= 0 else 0) for r in res)
                assert paths[4:] == sl.ratio_test_paths(lib_path=lib_path)[:4] or den != 1        # the same selection
                # den = 1 and a zero bound: no product is formed; den = 7: one-digit products in a lane, the wide ones in registers
                assert paths[0] == (sum(r[2] for r in res) if den == 1 else 0), paths
    assert any(r[0] < 0 for r in res) and any(r[0] >= 0 for r in res)


def check_reduction_on_handle(lib_path, name="test_mat", **kw):
    """on a handle: the same results and, with den = 1, the same winners' slab as Factorization.ratio_test"""
    import slip_lu_amd as sl
    _, fix = load_case(name)
    n, Ap, Ai, Alen, Alimbs, q = len(fix["q"]), fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"]
    cols = columns(n, Ap, Ai, oracle_lib.bigints(Alen, Alimbs))
    probs = handle_problems(n, cols, q, 11)
    b = slab([v for x, a in probs for side in (x, a) for v in side])
    key = np.array([(7 * i) % 5 for i in range(n)], np.int32)
    f = sl.Factorization(n, Ap, Ai, Alen, Alimbs, q, lib_path=lib_path, **kw)
    try:
        f.run(0)
        for den in (1, 7):
            bounds = sl.Bounds(n, np.ones(n, np.int32), slab([0] * n), None, den)
            for transpose in (False, True):
                for sense, k in ((1, None), (-1, key)):
                    old = f.ratio_test(*b, nprob=len(probs), transpose=transpose, sense=sense, key=k, winners=True)
                    new = f.ratio_test_bounded(*b, bounds, nprob=len(probs), transpose=transpose, sense=sense, key=k, winners=True)
                    assert all(np.array_equal(u, v) for u, v in zip(old[:3], new[:3])), (den, transpose, sense)
                    assert [int(s) for s in new[3]] == [-1 if int(v) >= 0 else 0 for v in new[0]]
                    if den == 1:
                        assert np.array_equal(old[3], new[4]) and np.array_equal(old[4], new[5])
                    assert f.bound_paths()[4:] == f.ratio_test_paths()[:4] or den != 1
                    assert min(f.bound_ms()) >= 0
    finally:
        f.close()


# ---- 2. width classes of the form pass ----

WIDTH_BD = 2 ** 70                                                 # three digits
WIDTH_LO = (TOP - 5) * B ** 29 + 12345                             # 30 digits, odd
WIDTH_HI = WIDTH_LO + 2
WIDTH_KIND = [1, 3, 1, 2, 0, 3, 1, 2, 3]


def width_bounds():
    """entry 0: a lower bound of 30 digits; entry 1: lower and upper bound the same 30-digit number; the others zero bounds"""
    return dict(kind=WIDTH_KIND, lo=[WIDTH_LO, WIDTH_HI] + [0] * 7, hi=[0, WIDTH_HI] + [0] * 7, den=WIDTH_BD)


def width_problem(W, upper):
    """n = 9, one d of W - 30 digits.  Entry 0: bd * x0 and d * lo0 have exactly W digits and differ by 3, in the lowest digit
    only (full-width cancellation).  Entry 1: bd * x1 = 2^30 * B^(W-1), all digits below the top zero, against d * hi1 a little
    below it: the subtraction borrows through every digit; `upper` sends it to its upper bound (a < 0), else to its lower
    bound of the same value.  The others: zero bounds and one-digit numerators, finished in a lane."""
    M = 2 ** 30 * B ** (W - 1)                                      # (no operand pair's bit lengths add up to more than 32 W)
    # bd | d * lo0 - 3 needs d = 3 / lo0 (mod bd), lo0 being odd; among those the d with d * hi1 just below M
    d0 = (3 * pow(WIDTH_LO, -1, WIDTH_BD)) % WIDTH_BD
    d = M // WIDTH_HI
    d -= (d - d0) % WIDTH_BD
    x0, x1 = (d * WIDTH_LO - 3) // WIDTH_BD, M // WIDTH_BD
    assert WIDTH_BD * x0 - d * WIDTH_LO == -3 and WIDTH_BD * x1 == M
    assert digits(WIDTH_BD * x0) == W == digits(d * WIDTH_LO) and (WIDTH_BD * x0) >> 32 == (d * WIDTH_LO) >> 32
    assert digits(d * WIDTH_HI) == W and 0 < M - d * WIDTH_HI < B ** 34
    avs = [5, -3 if upper else 3] + [(-1) ** k * (k + 1) for k in range(7)]
    xs = [x0, x1] + [(-1) ** k * 7 * (k + 2) for k in range(7)]    # (inside their zero bounds: positive steps, far above)
    return xs, avs, d


def check_width_classes(lib_path):
    bnd = width_bounds()
    probs = [width_problem(W, i % 2 == 0) for i, W in enumerate(BORDER_W)]
    singles = []
    for W, pr in zip(BORDER_W, probs):
        for sense, p in ((1, pr), (-1, (pr[0], [-a for a in pr[1]], pr[2]))):
            paths, res, _ = run_ratio(lib_path, [p], bnd, sense)
            # the two wide entries on the memory path above 256 digits, in registers otherwise; the others in a lane
            assert paths[3] == (2 if W > 256 else 0) and paths[2] == (0 if W > 256 else 2), (W, paths)
            assert paths[0] == 0 and paths[1] == res[0][2] - 2, (W, paths)
            if sense == 1:
                singles.append(res[0])
    assert {r[3] for r in singles} == {-1, 1}                      # both sides win somewhere
    paths, res, _ = run_ratio(lib_path, probs, bnd, 1)             # all classes in one call: the same results
    assert res == singles
    wide = sum(1 for W in BORDER_W if W > 256)
    assert paths[3] == 2 * wide and paths[2] == 2 * (len(BORDER_W) - wide)
    # operands of at most two digits: everything in a lane; bd = 1 and zero bounds: no product at all
    small = dict(kind=[1, 2, 3, 1, 2, 3, 0, 1, 2], lo=[B + 1, 0, -7, 2 ** 40, 0, 5, 1, -B, 3], hi=[0, 9, B + 5, 0, -(2 ** 33), 5, 1, 0, 2 ** 63], den=B + 3)
    sx, sa = [2 ** 50, -3, 11, B + 9, 4, -2 ** 62, 1, 0, 7], [3, -(B + 1), 5, -2, -7, 2 ** 40, 1, 9, -B]
    for d in (2 ** 33 + 1, -5):
        paths, res, _ = run_ratio(lib_path, [(sx, sa, d)], small, 1)
        assert paths[:4] == [0, res[0][2], 0, 0] and res[0][2] >= 3, paths
    unit = dict(kind=[1, 2, 3] * 3, lo=[0] * 9, hi=[0] * 9, den=1)
    paths, res, _ = run_ratio(lib_path, [(sx[:2] + [2 ** 300 + 1] + sx[3:], sa, -(2 ** 200))], unit, -1)
    assert paths[:4] == [res[0][2], 0, 0, 0] and res[0][2] > 3, paths


# ---- 3. signs, zeros, sides ----

def check_signs_and_sides(lib_path):
    wide, huge = 2 ** 200 + 3, 3 * B ** 66 + 1                     # 200 bits; more than 64 digits
    kind = [1, 2, 3, 0, 1, 2, 3, 0, 3, 3, 1, 2, 3, 3, 1, 2]
    lo = [12, 9, -4, 1, wide, 7, 10, 0, huge, -3, 6, 0, 5, 2, -wide, 0]
    hi = [8, 2, 6, 1, 0, wide, 3, 0, huge + 5, 3, 0, -huge, 5, 2, 0, 18]
    bnd = dict(kind=kind, lo=lo, hi=hi, den=6)
    n = len(kind)
    # x = d * bound / den puts an entry exactly on its bound: 12/6 = 2, 18/6 = 3, 6/6 = 1
    cases = [
        # d = 5: entries 0 and 10 on their lower bounds, 15 on its upper bound (N = 0, ratio 0), everything else above
        ([10, 0, 20, 1, wide, 0, 20, 0, huge, 0, 5, -huge, 9, 0, 0, 15], [3, -2, 5, 7, wide, -4, 0, -1, 2 ** 70, -6, 6, -2 ** 64, 1, -1, 9, -2], 5),
        # x below, on and above its bounds, wide operands on both sides, d = -5
        ([-11, 30, -2, 0, -wide - 1, wide, -50, 3, -huge * 2, 7, -5, huge, 1, -1, wide, -15], [-3, 2, -5, 7, wide, -wide, 1, -1, huge, 6, -6, 2 ** 64, -1, 1, 0, 2], -5),
        # a wide d; and nothing eligible: every a of the sign whose bound is missing, or zero
        ([wide, -wide, huge, 0, 1, -1, 7, 0, -huge, 2, 3, 4, 0, 0, 5, 6], [1, -1, wide, 3, -wide, huge, -7, 0, 2, -2, 5, -5, 1, -1, 3, 4], wide + 2),
        ([1] * n, [-1, 1, 0, 5, -2, 3, 0, 7, 0, 0, -1, 1, 0, 0, -4, 9], 7),
    ]
    seen = dict(lower=0, upper=0, missing=0, zero_tie=0, empty=0)
    for pad in (False, True):
        for sense in (1, -1):
            for key in (None, np.array([(5 * i) % 7 for i in range(n)], np.int32)):
                _, res, ties = run_ratio(lib_path, cases, bnd, sense, key, pad)
                for (xs, avs, d), r, tie in zip(cases, res, ties):
                    el = oracle_steps(xs, avs, d, bnd, sense)
                    seen["lower"] += r[3] == -1; seen["upper"] += r[3] == 1; seen["empty"] += r[0] < 0
                    seen["missing"] += any(a != 0 and i not in el and kind[i] not in (0, 3) for i, a in enumerate(avs))
                    seen["zero_tie"] += len(tie) > 1 and el[tie[0]][0] == 0
    assert all(seen.values()), seen
    assert lo[6] > hi[6]                                           # l > u is allowed


# ---- 4. exact ties in unreduced form ----

def check_ties(lib_path):
    p, q, den = 2 ** 61 - 1, 2 ** 45 + 59, 3
    ks = [3, 2 ** 40 + 15, 2 ** (32 * 33) - 5, 2 ** (32 * 70 - 7) + 9]           # 1, 2, 33 and 70 digits
    assert [digits(k) for k in ks] == [1, 2, 33, 70]
    big = ks[2]
    # N = k p (+-1) over a' = k q, the group alternating between the lower and the upper side
    ents = [(ks[3] * p, ks[3] * q, -1), (big * p + 1, big * q, 1), (ks[0] * p, ks[0] * q, 1), (big * p - 1, big * q, -1),
            (ks[2] * p, ks[2] * q, -1), (ks[1] * p, ks[1] * q, 1)]
    for d in (7, -(2 ** 64) - 7):
        kind, lo, hi, xs, avs = [], [], [], [], []
        for t, (N, a, side) in enumerate(ents):
            # lower: den * x - d * lo = N; upper: d * hi - den * x = N: a bound of the size of N with den | N + d * bound;
            # N carries the sign of d (N / d is the true distance to the bound)
            N = N if d > 0 else -N
            bound = N // 5 + t
            while ((N if side < 0 else -N) + d * bound) % den:
                bound += 1
            x = ((N if side < 0 else -N) + d * bound) // den
            kind.append(1 if side < 0 else 2); lo.append(bound if side < 0 else 0); hi.append(bound if side > 0 else 0)
            xs.append(x)
            avs.append((a if side < 0 else -a) * (1 if d > 0 else -1))                        # sense = 1: t > 0 on the lower side
        bnd = dict(kind=kind, lo=lo, hi=hi, den=den)
        with_above = [0, 1, 2, 4, 5]                               # the four-fold tie and the entry one unit above
        with_both = [0, 1, 2, 3, 4]                                # the entry one unit below wins alone
        sub = lambda idx: (dict(kind=[kind[i] for i in idx], lo=[lo[i] for i in idx], hi=[hi[i] for i in idx], den=den),
                           ([xs[i] for i in idx], [avs[i] for i in idx], d))
        for idx, want in ((with_above, (4, {-1, 1})), (with_both, (1, {-1}))):
            b, pr = sub(idx)
            for key in (None, [4, 3, 2, 1, 0], [7, 0, 7, 1, 1]):
                k = None if key is None else np.array(key, np.int32)
                for sense in (1, -1):
                    signed = pr if sense == 1 else (pr[0], [-a for a in pr[1]], pr[2])
                    paths, res, ties = run_ratio(lib_path, [signed], b, sense, k)
                    assert res[0][1] == want[0] and {ents[idx[i]][2] for i in ties[0]} == want[1], (d, key, sense)
                    assert paths[6] > 0                                               # the selection formed products


# ---- 5. geometry ----

def check_geometry(lib_path, sizes):
    rng = random.Random(5)
    for n in sizes:
        kind = [rng.randrange(4) for _ in range(n)]
        lo = [rng.randrange(-9, 10) * rng.choice((1, 1, B)) for _ in range(n)]
        hi = [v + rng.randrange(-2, 9) for v in lo]
        bnd = dict(kind=kind, lo=lo, hi=hi, den=rng.choice((1, 4, B + 1)))
        probs = [([rng.randrange(-40, 41) for _ in range(n)], [rng.choice((0, 1, -1, 1, -1)) * rng.randrange(1, 9) for _ in range(n)],
                  rng.choice((1, -3, 2 ** 40 + 1))) for _ in range(3)]
        key = np.array([rng.randrange(4) for _ in range(n)], np.int32)
        for sense in (1, -1):
            first = run_ratio(lib_path, probs, bnd, sense, key)
            assert run_ratio(lib_path, probs, bnd, sense, key) == first             # called twice: the same
        run_ratio(lib_path, probs, bnd, 1)
        vecs = [(xs, d) for xs, _, d in probs]
        first = run_bound(lib_path, vecs, bnd, key)
        assert run_bound(lib_path, vecs, bnd, key) == first
        run_bound(lib_path, vecs, bnd)


# ---- 6. the bound test ----

def check_bound_test(lib_path):
    wide = 2 ** 200 + 3
    kind = [3, 1, 2, 0, 3, 3, 1, 2, 3, 3]
    lo = [6, 12, 0, 5, -18, 30, wide * 6, 0, 12, -6]
    hi = [18, 0, 24, 5, 6, 6, 0, -wide * 6, 12, 36]               # entry 5: l = 5 > u = 1; entry 8: l = u = 2
    bnd = dict(kind=kind, lo=lo, hi=hi, den=6)
    n = len(kind)
    feasible = [2, 2, 4, 99, -3, None, wide, -wide, 2, 6]         # true values; entries 1, 2, 6, 7, 8 exactly on a bound
    for d in (5, -5, wide + 1):
        at = lambda vals: ([v * d for v in vals], d)
        ok = list(feasible); ok[5] = 0
        sub = dict(kind=kind[:5] + [0] + kind[6:], lo=lo, hi=hi, den=6)      # without the entry whose box is empty
        _, res, _ = run_bound(lib_path, [at(ok)], sub)
        assert res == [(-1, 0, 0, 0)]
        # the largest violation on the lower side (entry 1, by 7), on the upper side (entry 2, by 9); l > u: both sides are
        # violated, by 2 = l - x and 2 = x - u at x = 3, and the lower side is reported
        low = list(ok); low[1] = -5; low[0] = 0
        up = list(ok); up[2] = 13; up[9] = 7
        both = list(ok); both[5] = 3
        _, res, _ = run_bound(lib_path, [at(low), at(up), at(both), at(ok)], bnd)
        assert [r[0] for r in res] == [1, 2, 5, 5] and [r[3] for r in res] == [-1, 1, -1, -1]
        assert res[0][2] == 3 and res[2][1] == 1
    # equal violations in unreduced form: x_i = xnum_i / d against bounds over den, three entries violated by exactly 7/3
    d, den = 9, 6
    kind, lo, hi = [1, 2, 3, 1, 3], [12, 0, -6, 0, 0], [0, 12, 6, 0, 60]
    xs = [-3, 39, 30, -2, 89]                                      # 2 - (-1/3), 13/3 - 2, 10/3 - 1, 0 - (-2/9), 89/9 - 10 < 0
    bnd = dict(kind=kind, lo=lo, hi=hi, den=den)
    for key, best in ((None, 0), ([3, 2, 1, 0, 0], 2), ([1, 0, 0, 5, 5], 1)):
        for dd in (d, -d):
            _, res, ties = run_bound(lib_path, [([x * (1 if dd > 0 else -1) for x in xs], dd)], bnd, None if key is None else np.array(key, np.int32))
            assert res[0][:3] == (best, 3, 4) and ties[0] == [0, 1, 2]
    run_bound(lib_path, [(xs, d), ([-x for x in xs], d)], bnd, pad=True)
    # width classes as in the ratio test: entry 1 (l = u) is violated on the upper side by the little that is left when
    # two W-digit products cancel; one class in registers, one through memory
    wb = width_bounds()
    for W in (192, 300):
        xs, _, dd = width_problem(W, True)
        paths, res, _ = run_bound(lib_path, [(xs, dd)], wb)
        assert res[0][0] == 1 and res[0][3] == 1
        assert paths[3] == (2 if W > 256 else 0) and paths[2] == (0 if W > 256 else 2), (W, paths)
        _, res, _ = run_bound(lib_path, [(xs, -dd)], wb)
        assert res[0][0] >= 0


# ---- 7. on handles ----

def handle_bounds(n, xs, avs, det, sense, shift, on_bound):
    """bounds built from a problem's own numerators, den = |det|, kind[i] = (i + shift) mod 4: a group of up to two entries
    heading for their lower and two for their upper bound (three at least) ties exactly at the step tau = 3, every other eligible entry lies above
    it; on_bound: one eligible entry sits exactly on its bound instead (step 0).  Returns (bounds, group)."""
    s = 1 if det > 0 else -1
    tau = 3
    kind = [(i + shift) % 4 for i in range(n)]
    lo, hi = [0] * n, [0] * n
    lower = [i for i in range(n) if sense * s * avs[i] > 0 and kind[i] & 1]
    upper = [i for i in range(n) if sense * s * avs[i] < 0 and kind[i] & 2]
    group = sorted(lower[:2] + upper[:2])
    if not (lower and upper and len(group) >= 3):
        return None, None                                          # (this a side will not do: an empty entering column, say)
    for i in lower:
        lo[i] = s * xs[i] - (tau if i in group else tau + 1 + i % 3) * abs(avs[i])
    for i in upper:
        hi[i] = s * xs[i] + (tau if i in group else tau + 1 + i % 3) * abs(avs[i])
    if on_bound:
        group = [upper[-1]]
        hi[upper[-1]] = s * xs[upper[-1]]
    assert len(lower) + len(upper) < sum(1 for a in avs if a)      # some entry is held back by a missing bound
    return dict(kind=kind, lo=lo, hi=hi, den=abs(det)), group


def check_handle(f, n, probs, memory_path=False, light=False, transposes=(False, True)):
    """ratio_test_bounded and bound_test on a complete handle, against its own solve and the oracle.  Per orientation and per
    combination of sense and key two calls of two problems each: kind[i] = i mod 4 with a tie group at the step 3, and kind
    shifted by one with one entry exactly on its bound; the bounds of a call are built from the numerators of its first
    problem and the second problem shares them.  light (the emulator): one combination and one call per orientation;
    memory_path (the widest golden): half of the combinations, as ratio_helpers.check_handle, one call each, and the bound
    test in one orientation."""
    flat = [v for x, a in probs for side in (x, a) for v in side]
    b = slab(flat)
    det = oracle_lib.bigints(*f.pivots())[-1]
    key = np.array([(7 * i) % 5 for i in range(n)], np.int32)
    reached = 0
    for transpose in transposes:
        num = oracle_lib.bigints(*(f.solve_transpose if transpose else f.solve)(*b, nrhs=2 * len(probs)))
        sides = [(num[2 * c * n:(2 * c + 1) * n], num[(2 * c + 1) * n:(2 * c + 2) * n]) for c in range(len(probs))]
        for sense, k in ((1, None), (1, key), (-1, None), (-1, key)):
            if light and (sense, k is None) != ((1, False) if not transpose else (-1, True)):
                continue
            if memory_path and ((sense == 1) == (k is None)) == transpose:
                continue
            for call, (shift, on_bound) in enumerate(((0, False), (1, True))):
                if light and call != (1 if transpose else 0):
                    continue
                if memory_path and call != (0 if sense == 1 else 1):      # (a substitution there takes 0.3 s: one call a combination)
                    continue
                # the first problem, from `call` on, whose a side gives both signs among the eligible entries
                tries = [(c, handle_bounds(n, *sides[c], det, sense, shift, on_bound)) for c in [(call + t) % len(probs) for t in range(len(probs))]]
                first, (bnd, group) = next((t for t in tries if t[1][0] is not None), (None, (None, None)))
                assert bnd is not None, "no problem of this golden gives both signs of a among the eligible entries"
                order = [first] + [c for c in range(len(probs)) if c != first][:1]
                bb = slab([v for c in order for side in probs[c] for v in side])
                got = f.ratio_test_bounded(*bb, make_bounds(n, bnd), nprob=len(order), transpose=transpose, sense=sense, key=k, winners=True)
                els = [oracle_steps(*sides[c], det, bnd, sense) for c in order]
                want = [pick(el, k) for el in els]
                for t, what in enumerate(("best", "nties", "neligible", "side")):
                    assert [int(v) for v in got[t]] == [w[0][t] for w in want], (what, transpose, sense, call)
                same_slab(got[4:], [v for c, w in zip(order, want) for v in winner_ratio(*sides[c], det, bnd, w[0][0], w[0][3])],
                          "the winners' N and a'")
                # what the construction promises, as the oracle sees it
                assert sorted(want[0][1]) == group and want[0][0][1] == len(group)
                assert {side for _, side in els[0].values()} == {-1, 1}
                assert el_step(els[0], want[0][0][0]) == (0 if on_bound else 3)
                paths = f.bound_paths()
                assert sum(paths[:4]) == sum(w[0][2] for w in want) and paths[4] == sum(paths[:4])
                reached += paths[3]
        # the bound test on the x sides: boxes x_i +- small around the first vector, a third of them moved off it
        if memory_path and transpose:
            continue                                               # (one orientation where a substitution takes 0.3 s)
        s = 1 if det > 0 else -1
        xs = sides[0][0]
        kind = [3 if i % 5 else 1 + i % 2 for i in range(n)]
        lo = [s * x - (2 + i % 3) * abs(det) for i, x in enumerate(xs)]
        hi = [s * x + (2 + i % 4) * abs(det) for i, x in enumerate(xs)]
        moved = [i for i in range(n) if i % 3 == 0]
        for r, i in enumerate(moved):                              # violated by 1 + r % 3 units; two entries tie for the worst, 5
            v = (5 if r in (1, len(moved) - 1) else 1 + r % 3) * abs(det)
            if kind[i] & 1 and (r % 2 == 0 or not kind[i] & 2):
                lo[i] = s * xs[i] + v
                hi[i] = max(hi[i], lo[i] + 1)
            else:
                hi[i] = s * xs[i] - v
                lo[i] = min(lo[i], hi[i] - 1)
        bnd = dict(kind=kind, lo=lo, hi=hi, den=abs(det))
        xb = slab([v for c in (0, len(probs) - 1) for v in probs[c][0]])
        for k in ((None,) if light or memory_path else (None, key)):
            got = f.bound_test(*xb, make_bounds(n, bnd), nprob=2, transpose=transpose, key=k, winners=True)
            els = [oracle_violations(sides[c][0], det, bnd) for c in (0, len(probs) - 1)]
            want = [pick(el, k, largest=True) for el in els]
            for t, what in enumerate(("worst", "nties", "nviolated", "side")):
                assert [int(v) for v in got[t]] == [w[0][t] for w in want], (what, transpose)
            same_slab(got[4:], [winner_violation(el, det, bnd, w[0][0]) for el, w in zip(els, want)], "the worst violations")
            assert want[0][0][2] == len(moved) and (want[0][0][1] == 2 or len(moved) < 3)
            reached += f.bound_paths()[3]
    if memory_path:
        assert reached > 0, "the memory path of the form pass was not reached"
    return det


def el_step(el, best):
    return el[best][0]


def check_golden(lib_path, name, memory_path=False, light=False, transposes=(False, True), **kw):
    import slip_lu_amd as sl
    _, fix = load_case(name)
    n, Ap, Ai, Alen, Alimbs, q = len(fix["q"]), fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"]
    cols = columns(n, Ap, Ai, oracle_lib.bigints(Alen, Alimbs))
    f = sl.Factorization(n, Ap, Ai, Alen, Alimbs, q, lib_path=lib_path, **kw)
    try:
        f.run(0)
        probs = handle_problems(n, cols, q, 11)
        # (the emulator and the widest golden take the first and the last problem, as ratio_helpers.check_golden does)
        check_handle(f, n, probs[::2] if light or memory_path else probs, memory_path, light, transposes)
    finally:
        f.close()


# ---- 8. a handle with a negative determinant; the handle's other services afterwards ----

def check_negative_det(lib_path, name="gen_n40", light=False, **kw):
    """ratio_helpers.check_negative_det's handle (one column negated when the golden's det is positive); afterwards solve,
    ratio_test and multiply return what a fresh handle returns"""
    import slip_lu_amd as sl
    _, fix = load_case(name)
    n, Ap, Ai, Alen, Alimbs, q = len(fix["q"]), fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"]
    Alen = np.array(Alen, np.int32).copy()
    f = sl.Factorization(n, Ap, Ai, Alen, Alimbs, q, lib_path=lib_path, **kw)
    try:
        f.run(0)
        det = oracle_lib.bigints(*f.pivots())[-1]
    finally:
        f.close()
    if det > 0:
        j = int(q[0])
        Alen[int(Ap[j]):int(Ap[j + 1])] *= -1
    cols = columns(n, Ap, Ai, oracle_lib.bigints(Alen, Alimbs))
    f = sl.Factorization(n, Ap, Ai, Alen, Alimbs, q, lib_path=lib_path, **kw)
    g = sl.Factorization(n, Ap, Ai, Alen, Alimbs, q, lib_path=lib_path, **kw)
    try:
        f.run(0); g.run(0)
        probs = handle_problems(n, cols, q, 12)
        probs = probs[::2] if light else probs
        assert check_handle(f, n, probs, light=light, transposes=(False,) if light else (False, True)) < 0
        b = slab([v for x, a in probs for side in (x, a) for v in side])
        rhs = slab(probs[0][0])
        for what in (lambda h: h.solve(*rhs), lambda h: h.solve_transpose(*rhs), lambda h: h.ratio_test(*b, nprob=len(probs), winners=True),
                     lambda h: h.multiply(*h.solve(*rhs))):
            assert all(np.array_equal(u, v) for u, v in zip(what(f), what(g)))
    finally:
        f.close(); g.close()


# ---- 9. rejections: SLIP_HIP_INCORRECT_INPUT (-3), nothing written ----

def check_rejections(lib_path, name="test_mat", **kw):
    import slip_lu_amd as sl
    from slip_lu_amd import _lib
    lib = _lib.load(lib_path)
    n = 3
    xl, xv = slab([5, -(2 ** 64), 1]); al, av = slab([1, 2 ** 64 + 1, -3]); dl, dv = slab([7]); zl, zv = np.zeros(1, np.int32), np.zeros(1, np.uint64)
    kind = np.array([1, 2, 3], np.int32)
    bl, bv = slab([1, 2 ** 64, -2])
    den = np.array([6], np.uint64)
    res = [np.full(2, 77, np.int32) for _ in range(4)]
    R = [r.ctypes.data for r in res]
    pl, px, nl = C.c_void_p(), C.c_void_p(), C.c_int64()
    outs = (C.byref(pl), C.byref(px), C.byref(nl))

    def rec(kind=kind, lo=(bl, bv, bv.size), hi=(bl, bv, bv.size), bd=(1, den)):
        r = _lib.BoundsRec()
        r.keep = (kind, lo, hi, bd)                                # (the record holds addresses only)
        r.kind = None if kind is None else kind.ctypes.data
        if lo is not None:
            r.lolen, r.lolimbs, r.lo_limbs = lo[0].ctypes.data, lo[1].ctypes.data, lo[2]
        if hi is not None:
            r.hilen, r.hilimbs, r.hi_limbs = hi[0].ctypes.data, hi[1].ctypes.data, hi[2]
        if bd is not None:
            r.bdlen, r.bdlimbs = bd[0], bd[1].ctypes.data
        return r

    X_, A_, D_ = (xl.ctypes.data, xv.ctypes.data, xv.size), (al.ctypes.data, av.ctypes.data, av.size), (dl.ctypes.data, dv.ctypes.data, dv.size)
    good = rec()
    bad_bounds = [None, rec(kind=None), rec(kind=np.array([1, 4, 0], np.int32)), rec(kind=np.array([-1, 0, 0], np.int32)),
                  rec(lo=None), rec(hi=None), rec(lo=(bl, bv, bv.size - 1)), rec(hi=(bl, bv, bv.size - 1)),
                  rec(bd=(0, den)), rec(bd=(-1, den)), rec(bd=(1, np.zeros(1, np.uint64)))]
    ref = lambda r: None if r is None else C.byref(r)
    ratio, bound = lib.slip_hip_ratio_test_bounded, lib.slip_hip_bound_test
    for r in bad_bounds:
        assert ratio(n, 1, *X_, *A_, *D_, ref(r), 1, None, *R, *outs, None) == -3
        assert bound(n, 1, *X_, *D_, ref(r), None, *R, *outs, None) == -3
    g = C.byref(good)
    bad = [(0, 1, *X_, *A_, *D_, g, 1, None, *R, *outs, None), (n, 0, *X_, *A_, *D_, g, 1, None, *R, *outs, None),
           (n, 1, *X_, *A_, *D_, g, 0, None, *R, *outs, None), (n, 1, *X_, *A_, *D_, g, 2, None, *R, *outs, None),
           (n, 1, None, X_[1], X_[2], *A_, *D_, g, 1, None, *R, *outs, None), (n, 1, *X_, A_[0], None, A_[2], *D_, g, 1, None, *R, *outs, None),
           (n, 1, *X_, None, None, 0, *D_, g, 1, None, *R, *outs, None), (n, 1, *X_, *A_, None, None, 0, g, 1, None, *R, *outs, None),
           (n, 1, X_[0], X_[1], X_[2] - 1, *A_, *D_, g, 1, None, *R, *outs, None), (n, 1, *X_, A_[0], A_[1], A_[2] - 1, *D_, g, 1, None, *R, *outs, None),
           (n, 1, *X_, *A_, D_[0], D_[1], 0, g, 1, None, *R, *outs, None),
           (n, 1, *X_, *A_, zl.ctypes.data, zv.ctypes.data, 1, g, 1, None, *R, *outs, None),                     # d = 0
           (n, 1, *X_, *A_, *D_, g, 1, None, None, R[1], R[2], R[3], *outs, None), (n, 1, *X_, *A_, *D_, g, 1, None, R[0], R[1], R[2], None, *outs, None),
           (n, 1, *X_, *A_, *D_, g, 1, None, *R, outs[0], None, outs[2], None), (n, 1, *X_, *A_, *D_, g, 1, None, *R, None, None, outs[2], None)]
    for args in bad:
        assert ratio(*args) == -3, args[:2]
    bad = [(0, 1, *X_, *D_, g, None, *R, *outs, None), (n, 0, *X_, *D_, g, None, *R, *outs, None),
           (n, 1, X_[0], None, X_[2], *D_, g, None, *R, *outs, None), (n, 1, X_[0], X_[1], X_[2] - 1, *D_, g, None, *R, *outs, None),
           (n, 1, *X_, zl.ctypes.data, zv.ctypes.data, 1, g, None, *R, *outs, None),
           (n, 1, *X_, *D_, g, None, R[0], None, R[2], R[3], *outs, None), (n, 1, *X_, *D_, g, None, *R, outs[0], outs[1], None, None)]
    for args in bad:
        assert bound(*args) == -3, args[:2]
    assert all((r == 77).all() for r in res) and pl.value is None and px.value is None
    assert lib.slip_hip_bound_paths(None) == -3
    # a side nothing switches on may be NULL; a denominator of NULL limbs is 1; the good record is accepted
    assert ratio(n, 1, *X_, *A_, *D_, ref(rec(kind=np.array([1, 0, 1], np.int32), hi=None, bd=None)), 1, None, *R, None, None, None, None) == 0
    assert bound(n, 1, *X_, *D_, g, None, *R, None, None, None, None) == 0
    with pytest.raises(ValueError):
        sl.Bounds(4, kind)
    with pytest.raises(ValueError):
        sl.ratio_test_bounded(2, xl, xv, al, av, dl, dv, sl.Bounds(3, kind, (bl, bv), (bl, bv)), lib_path=lib_path)
    # on a handle
    _, fix = load_case(name)
    n, Ap, Ai, Alen, Alimbs, q = len(fix["q"]), fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"]
    b = slab([(-1) ** t * (t % 7) for t in range(2 * n)])
    hl, hv = b[0].ctypes.data, b[1].ctypes.data
    bounds = sl.Bounds(n, np.array([i % 4 for i in range(n)], np.int32), slab(list(range(n))), slab(list(range(3, n + 3))), 5)
    hb = bounds.ref(n)
    res = [np.full(2, 77, np.int32) for _ in range(4)]
    R = [r.ctypes.data for r in res]
    f = sl.Factorization(n, Ap, Ai, Alen, Alimbs, q, lib_path=lib_path, **kw)
    try:
        f.run(n // 2)
        assert f.info()["K"] < n
        for call in (lambda: f.ratio_test_bounded(*b, bounds), lambda: f.bound_test(b[0][:n], b[1], bounds)):
            with pytest.raises(sl.SlipError) as e:                # an incomplete factorisation
                call()
            assert e.value.code == -3
        f.run(0)
        fr, fb = lib.slip_hip_factor_ratio_test_bounded, lib.slip_hip_factor_bound_test
        bad = [(None, 0, 1, hl, hv, hb, 1, None, *R, *outs, None), (f.h, 0, 0, hl, hv, hb, 1, None, *R, *outs, None),
               (f.h, 0, 1, None, hv, hb, 1, None, *R, *outs, None), (f.h, 0, 1, hl, None, hb, 1, None, *R, *outs, None),
               (f.h, 0, 1, hl, hv, None, 1, None, *R, *outs, None), (f.h, 0, 1, hl, hv, hb, 0, None, *R, *outs, None),
               (f.h, 1, 1, hl, hv, hb, -2, None, *R, *outs, None), (f.h, 0, 1, hl, hv, hb, 1, None, R[0], R[1], R[2], None, *outs, None),
               (f.h, 0, 1, hl, hv, hb, 1, None, *R, outs[0], None, outs[2], None)]
        for args in bad:
            assert fr(*args) == -3, args[1:3]
        bad = [(None, 0, 1, hl, hv, hb, None, *R, *outs, None), (f.h, 0, 0, hl, hv, hb, None, *R, *outs, None),
               (f.h, 0, 1, hl, hv, None, None, *R, *outs, None), (f.h, 0, 1, hl, hv, hb, None, None, R[1], R[2], R[3], *outs, None),
               (f.h, 1, 1, hl, hv, hb, None, *R, None, outs[1], outs[2], None)]
        for args in bad:
            assert fb(*args) == -3, args[1:3]
        wrong = sl.Bounds(n, np.array([i % 5 for i in range(n)], np.int32), slab(list(range(n))), slab(list(range(n))))
        assert fr(f.h, 0, 1, hl, hv, wrong.ref(n), 1, None, *R, *outs, None) == -3                # a kind of 4
        assert all((r == 77).all() for r in res) and pl.value is None and px.value is None
        assert lib.slip_hip_factor_bound_paths(f.h, None) == -3 and lib.slip_hip_factor_bound_ms(None, R[0]) == -3
        with pytest.raises(ValueError):
            f.ratio_test_bounded(*b, bounds, nprob=2)
        with pytest.raises(ValueError):
            f.bound_test(*b, bounds, key=np.zeros(n + 1, np.int32))
        fac = f.download()
        tr = f.ratio_test_bounded(*b, bounds, transpose=True, winners=True)
        tb = f.bound_test(b[0][:n], b[1], bounds, transpose=True, winners=True)
    finally:
        f.close()
    g = sl.Factorization.from_factors(fac, lib_path=lib_path, **{k: v for k, v in kw.items() if k in ("waves", "workers")})
    try:
        for call in (lambda: g.ratio_test_bounded(*b, bounds), lambda: g.bound_test(b[0][:n], b[1], bounds)):
            with pytest.raises(sl.SlipError) as e:                # a handle around given factors holds no q
                call()
            assert e.value.code == -3
        assert all(np.array_equal(u, v) for u, v in zip(g.ratio_test_bounded(*b, bounds, transpose=True, winners=True), tr))
        assert all(np.array_equal(u, v) for u, v in zip(g.bound_test(b[0][:n], b[1], bounds, transpose=True, winners=True), tb))
    finally:
        g.close()
