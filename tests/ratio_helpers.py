"""Shared by tests/test_emu_ratio.py (the emulator build) and tests/test_gpu_ratio.py (the product on the device): the exact
ratio test (slip_hip_ratio_test on two slabs, slip_hip_factor_ratio_test fused with a solve on a handle).  The oracle is
Python: Fraction(x_i, sense * a_i) over the eligible entries, min by (ratio, key, i), and counting; every comparison is exact
equality.  lib_path None is the product library."""
import ctypes as C
import random
from fractions import Fraction

import numpy as np
import pytest

import oracle_lib
from check_helpers import columns, slab
from conftest import load_case
from product_helpers import BORDER_W, same_slab

B = 2 ** 32
TOP = B - 1


# ---- the oracle ----

def oracle_ties(xs, avs, sense, dsign=1, fr=None):
    """(the eligible entries whose ratio is the minimum, neligible) of one problem.  avs None: no denominators, every entry
    eligible, ratio sense * x.  dsign: the sign of the common denominator both sides were multiplied by (a handle's det): it
    counts for the eligibility only.  fr: Fraction(x_i, a_i) of the entries with a_i != 0, formed once by the caller
    (x_i / (sense * a_i) is sense times it)."""
    n = len(xs)
    if avs is None:
        el = list(range(n))
        r = {i: Fraction(sense * xs[i]) for i in el}
    else:
        el = [i for i in range(n) if sense * dsign * avs[i] > 0]
        r = {i: sense * fr[i] if fr is not None else Fraction(xs[i], sense * avs[i]) for i in el}
    if not el:
        return [], 0
    m = min(r.values())
    return [i for i in el if r[i] == m], len(el)


def pick(ties, neligible, key=None):
    """(best, nties, neligible): among the ties the smallest (key, i)"""
    if not ties:
        return -1, 0, 0
    return min(ties, key=lambda i: (int(key[i]) if key is not None else 0, i)), len(ties), neligible


def oracle(xs, avs, sense, key=None, dsign=1, fr=None):
    return pick(*oracle_ties(xs, avs, sense, dsign, fr), key)


def run(lib_path, probs, sense=1, key=None, denominators=True, pad=None):
    """one call of slip_hip_ratio_test on the problems [(xs, avs), ...], compared with the oracle; returns the path counts.
    pad: per flat entry, high zero limbs to append (un-normalised input)."""
    import slip_lu_amd as sl
    n = len(probs[0][0])
    xlen, xlimbs = padded_slab([v for xs, _ in probs for v in xs], pad)
    a = padded_slab([v for _, avs in probs for v in avs], pad) if denominators else (None, None)
    got = sl.ratio_test(n, xlen, xlimbs, *a, nprob=len(probs), sense=sense, key=key, lib_path=lib_path)
    want = [oracle(xs, avs if denominators else None, sense, key) for xs, avs in probs]
    for t, what in enumerate(("best", "nties", "neligible")):
        assert [int(v) for v in got[t]] == [w[t] for w in want], (what, sense, key)
    return sl.ratio_test_paths(lib_path=lib_path)


def padded_slab(values, pad=None):
    """python ints -> (signed limb counts, limbs) with pad[t] high zero limbs appended to entry t (a zero entry keeps sign +)"""
    if pad is None:
        return slab(values)
    lens, limbs = [], []
    for v, extra in zip(values, pad):
        a, own = abs(int(v)), []
        while a:
            own.append(a & (2 ** 64 - 1)); a >>= 64
        own += [0] * extra
        lens.append(-len(own) if v < 0 else len(own))
        limbs += own
    return np.array(lens, np.int32), np.array(limbs, np.uint64)


# ---- 1. width classes: the two best ratios agree in their leading 64 bits and only the exact pass tells them apart ----

def width_problem(W, flip):
    """n = 9: p/q against (p M + 1)/(q M) (flip: p M - 1, so the long entry wins), cross products of W digits each
    (1 + (W - 1)), M of W - 2 digits all ones, and seven entries at least a factor 4 above, which the bound pass removes"""
    p, q, M = TOP, TOP - 2, B ** (W - 2) - 1
    xs = [p * 4 ** (k + 1) + k for k in range(7)]
    avs = [q] * 7
    xs[2:2] = [p]; avs[2:2] = [q]
    xs[6:6] = [p * M + (-1 if flip else 1)]; avs[6:6] = [q * M]
    return xs, avs


def check_width_classes(lib_path):
    probs = [width_problem(W, i % 2 == 1) for i, W in enumerate(BORDER_W)]
    formed = 0
    for W, (xs, avs) in zip(BORDER_W, probs):
        digits = lambda v: (abs(v).bit_length() + 31) // 32
        assert digits(xs[2]) + digits(avs[6]) == W == digits(xs[6]) + digits(avs[2])
        assert (xs[2] * avs[6]) >> (32 * W - 64) == (xs[6] * avs[2]) >> (32 * W - 64)       # equal leading 64 bits
        for sense, pr in ((1, (xs, avs)), (-1, (xs, [-v for v in avs]))):
            paths = run(lib_path, [pr], sense)
            assert paths[0] == 9 and paths[1] == 2 and paths[2] == 1, (W, paths)
            assert paths[3] == (1 if W > 256 else 0), (W, paths)
            formed += paths[2]
    assert formed > 0
    paths = run(lib_path, probs, 1)                                 # all classes in one call
    assert paths[1] == 2 * len(probs) and paths[2] == len(probs) and paths[3] == sum(1 for W in BORDER_W if W > 256)


# ---- 2. exact ties in unreduced form ----

def check_ties(lib_path):
    p, q = 2 ** 61 - 1, 2 ** 45 + 59
    ks = [3, 2 ** 40 + 15, 2 ** (32 * 33) - 5, 2 ** (32 * 70 - 7) + 9]           # 1, 2, 33 and 70 digits
    assert [(k.bit_length() + 31) // 32 for k in ks] == [1, 2, 33, 70]
    big = ks[2]
    tied = [(k * p, k * q) for k in ks]
    above = (big * p + 1, big * q)                                 # strictly larger, by one unit of the numerator
    below = (big * p - 1, big * q)                                 # strictly smaller by as much
    with_above = [tied[3], above, tied[0], tied[2], tied[1]]
    with_both = [tied[3], above, tied[0], below, tied[2]]
    probs = [([x for x, _ in pr], [a for _, a in pr]) for pr in (with_above, with_both)]
    for key in (None, [4, 3, 2, 1, 0], [7, 0, 7, 1, 1]):
        for sense in (1, -1):
            signed = probs if sense == 1 else [(xs, [-a for a in avs]) for xs, avs in probs]
            paths = run(lib_path, signed, sense, None if key is None else np.array(key, np.int32))
            assert paths[2] > 0
    assert oracle(*probs[0], 1)[:2] == (0, 4) and oracle(*probs[1], 1)[:2] == (3, 1)
    assert oracle(*probs[0], 1, [4, 3, 2, 1, 0])[0] == 4 and oracle(*probs[0], 1, [7, 0, 7, 1, 1])[0] == 3


# ---- 3. signs and zeros ----

def check_signs_and_zeros(lib_path):
    wide = 2 ** 200 + 3
    xs = [5, -7, wide, -wide, 0, 9, 0, -3, 11, 4, -4, 0]
    avs = [3, 2, -5, -wide, 7, 0, 0, -1, 2 ** 70, -6, 6, -2 ** 64]
    for sense in (1, -1):
        run(lib_path, [(xs, avs)], sense)
        run(lib_path, [(xs, avs)], sense, np.arange(12, dtype=np.int32)[::-1].copy())
    assert oracle(xs, avs, 1)[2] == 5 and oracle(xs, avs, -1)[2] == 5
    # un-normalised: high zero limbs on every entry, a zero written with two limbs
    pad = [t % 3 for t in range(12)]
    pad[4] = 2
    for sense in (1, -1):
        run(lib_path, [(xs, avs)], sense, pad=pad)
    # a degenerate vertex: many x_i = 0 with eligible a_i all tie at 0 and cost no product, however many they are
    counts = []
    for zeros in (5, 50):
        zx = [0] * zeros + [3, 2 ** 90, 1]
        za = [2 ** (7 * t) + 1 for t in range(zeros)] + [5, 7, -1]
        paths = run(lib_path, [(zx, za)], 1)
        assert oracle(zx, za, 1)[:2] == (0, zeros)
        counts.append(paths[2])
    assert counts[0] == counts[1] == 0
    # nothing eligible; and three problems with different winners, one of them empty
    run(lib_path, [([1, 2, 3], [-1, 0, -5])], 1)
    assert oracle([1, 2, 3], [-1, 0, -5], 1) == (-1, 0, 0)
    probs = [([4, 1, 9], [2, 1, 3]), ([1, 2, 3], [-1, 0, -5]), ([-8, -wide, 5], [1, 3, 1])]
    run(lib_path, probs, 1)
    assert [oracle(*pr, 1)[0] for pr in probs] == [1, -1, 1]
    run(lib_path, probs, -1)


# ---- 4. geometry ----

def check_geometry(lib_path, sizes):
    rng = random.Random(5)
    for n in sizes:
        # one-digit operands of both signs, a few zeros
        xs = [rng.choice((0, 1, -1, 1, 1)) * rng.randrange(1, B) for _ in range(n)]
        avs = [rng.choice((0, 1, -1, 1, 1)) * rng.randrange(1, B) for _ in range(n)]
        ys = [rng.choice((1, -1)) * rng.randrange(1, B) for _ in range(n)]
        key = np.array([rng.randrange(4) for _ in range(n)], np.int32)
        for sense in (1, -1):
            first = run(lib_path, [(xs, avs), (ys, avs)], sense, key)
            assert run(lib_path, [(xs, avs), (ys, avs)], sense, key) == first                   # called twice: the same
        # all ratios equal (x_i = 5 t_i, a_i = 3 t_i): every entry is a candidate, the chunk fold and the final fold run
        ts = [rng.randrange(1, B // 8) for _ in range(n)]
        eq = ([5 * t for t in ts], [3 * t for t in ts])
        paths = run(lib_path, [eq], 1, key)
        assert oracle(*eq, 1)[1] == n and paths[1] == n and paths[2] == n - 1
        # all ratios pairwise at least a factor 4 apart: the bound pass leaves the winner alone.  (One-digit operands hold
        # only 32 such ratios, so the numerators grow here: x_i = 4^pi(i) * u with 1 <= u < 2 in 20 bits, a_i one digit.)
        order = list(range(n))
        rng.shuffle(order)
        far = ([(-1) ** (i % 2) * ((2 ** 20 + rng.randrange(2 ** 19)) << (3 * order[i])) for i in range(n)], [rng.randrange(2 ** 31, 2 ** 31 + 2 ** 28) for _ in range(n)])
        for sense in (1, -1):
            pr = (far[0], far[1] if sense == 1 else [-a for a in far[1]])
            paths = run(lib_path, [pr, (pr[0][::-1], pr[1][::-1])], sense)
            assert paths[1] == 2 and paths[2] == 0, (n, paths)


# ---- 5. no denominators: argmin / argmax of signed integers ----

def check_no_denominators(lib_path):
    wide = 2 ** 300 + 2 ** 64
    vecs = [[5, -3, 0, -3, 7, 7, 0],                                # repeated minima and maxima, zeros
            [wide + 1, wide, wide + 2, -wide, -wide - 1, -wide, wide + 2],      # multi-limb, differing in the lowest limb only
            [0, 0, 0, 0, 0, 0, 0]]
    for key in (None, np.array([1, 0, 0, 1, 0, 1, 0], np.int32)):
        for sense in (1, -1):
            run(lib_path, [(v, None) for v in vecs], sense, key, denominators=False)
    assert oracle(vecs[0], None, 1)[:2] == (1, 2) and oracle(vecs[0], None, -1)[:2] == (4, 2)
    assert oracle(vecs[1], None, 1)[:2] == (4, 1) and oracle(vecs[1], None, -1)[:2] == (2, 2)
    assert oracle(vecs[2], None, 1) == (0, 7, 7)
    pad = [t % 2 for t in range(21)]
    run(lib_path, [(v, None) for v in vecs], 1, denominators=False, pad=pad)


# ---- 6. on handles ----

def handle_problems(n, cols, q, seed):
    """three problems as right-hand sides (dense, n ints each): small random b against an entering column, twice, and a pair
    with x side = 3 * a side, where every eligible entry ties.  An entering column is a column of A moved down by one row (a
    column of A itself is in the basis: its alpha would be a unit vector)"""
    rng = random.Random(seed)
    entering = lambda j: [cols[j].get((i + 1) % n, 0) for i in range(n)]
    b0 = [rng.randrange(-9, 10) for _ in range(n)]
    b1 = [rng.randrange(-99, 100) for _ in range(n)]
    e0, e1 = entering(int(q[n // 3])), entering(int(q[n - 1]))
    mix = [u + v for u, v in zip(e0, b0)]
    return [(b0, e0), (b1, e1), ([3 * v for v in mix], mix)]


def check_handle(f, n, probs, memory_path=False, light=False, transposes=(False, True)):
    """every combination of transpose, sense and key on a complete handle, against its own solve and the oracle (light, for
    the emulator: one combination per orientation)"""
    flat = [v for x, a in probs for side in (x, a) for v in side]
    b = slab(flat)
    det = oracle_lib.bigints(*f.pivots())[-1]
    dsign = 1 if det > 0 else -1
    key = np.array([(7 * i) % 5 for i in range(n)], np.int32)
    reached = 0
    for transpose in transposes:
        num = oracle_lib.bigints(*(f.solve_transpose if transpose else f.solve)(*b, nrhs=2 * len(probs)))
        sides = [(num[2 * c * n:(2 * c + 1) * n], num[(2 * c + 1) * n:(2 * c + 2) * n]) for c in range(len(probs))]
        frs = [[Fraction(x, a) if a else None for x, a in zip(xs, avs)] for xs, avs in sides]
        tied = {sense: [oracle_ties(x, a, sense, dsign, fr) for (x, a), fr in zip(sides, frs)] for sense in (1, -1)}
        for sense, k in ((1, None), (1, key), (-1, None), (-1, key)):
            if light and (sense, k is None) != ((1, False) if not transpose else (-1, True)):
                continue
            if memory_path and ((sense == 1) == (k is None)) == transpose:
                continue                                           # (see check_golden: half of the combinations)
            want = [pick(*t, k) for t in tied[sense]]
            best, nties, nelig, wlen, wlimbs = f.ratio_test(*b, nprob=len(probs), transpose=transpose, sense=sense, key=k, winners=True)
            assert [(int(best[c]), int(nties[c]), int(nelig[c])) for c in range(len(probs))] == want, (transpose, sense)
            same_slab((wlen, wlimbs), [v for c, w in enumerate(want) for v in ((sides[c][0][w[0]], sides[c][1][w[0]]) if w[0] >= 0 else (0, 0))],
                      "the winners' numerators")
            paths = f.ratio_test_paths()
            assert paths[0] == sum(w[2] for w in want) and paths[1] >= sum(w[1] for w in want)
            assert f.ratio_test_ms() >= 0
            reached += paths[3]
        if not light and not memory_path:                          # without the winners' slab: the same three arrays
            plain = f.ratio_test(*b, nprob=len(probs), transpose=transpose, sense=sense, key=k)
            assert len(plain) == 3 and all(np.array_equal(u, v) for u, v in zip(plain, (best, nties, nelig)))
        # all ties in the last problem, under one sense or the other
        assert max(len(tied[s][-1][0]) for s in (1, -1)) > 1
    if memory_path:
        assert reached > 0, "the memory path (cross products above 256 digits) was not reached"
    return det


def check_golden(lib_path, name, memory_path=False, light=False, transposes=(False, True), **kw):
    import slip_lu_amd as sl
    _, fix = load_case(name)
    n, Ap, Ai, Alen, Alimbs, q = len(fix["q"]), fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"]
    cols = columns(n, Ap, Ai, oracle_lib.bigints(Alen, Alimbs))
    f = sl.Factorization(n, Ap, Ai, Alen, Alimbs, q, lib_path=lib_path, **kw)
    try:
        f.run(0)
        probs = handle_problems(n, cols, q, 11)
        # (the emulator and the widest golden, where one substitution takes 0.6 s on the device, take the first and the last
        # problem; that golden also takes half of the eight combinations -- plain with (+1, no key) and (-1, key), transposed
        # with (+1, key) and (-1, no key) -- which the four other goldens run in full)
        check_handle(f, n, probs[::2] if light or memory_path else probs, memory_path, light, transposes)
    finally:
        f.close()


def check_negative_det(lib_path, name="gen_n40", light=False, **kw):
    """a handle with det < 0, where the eligible sign of anum is the opposite of sense: when the golden's det is positive, one
    column is negated (the pivot search goes by magnitude, so the same pivots are chosen and det changes sign)"""
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
    try:
        f.run(0)
        assert oracle_lib.bigints(*f.pivots())[-1] < 0, "det must be negative on this handle"
        probs = handle_problems(n, cols, q, 12)
        assert check_handle(f, n, probs[::2] if light else probs, light=light) < 0
    finally:
        f.close()


# ---- 7. lifecycle ----

def check_lifecycle(lib_path, name="gen_n40", light=False, **kw):
    import slip_lu_amd as sl
    _, fix = load_case(name)
    n, Ap, Ai, Alen, Alimbs, q = len(fix["q"]), fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"]
    cols = columns(n, Ap, Ai, oracle_lib.bigints(Alen, Alimbs))
    probs = handle_problems(n, cols, q, 13)[:1]
    b = slab([v for x, a in probs for side in (x, a) for v in side])
    rhs = slab(probs[0][0])
    f = sl.Factorization(n, Ap, Ai, Alen, Alimbs, q, lib_path=lib_path, **kw)
    try:
        f.run(0)
        best, nties, nelig = f.ratio_test(*b)
        sense = 1
        if best[0] < 0:
            sense = -1
            best, nties, nelig = f.ratio_test(*b, sense=-1)
        p = int(best[0])
        assert 0 <= p < n
        # the column at the leaving position gets new content: the entering column plus a unit entry
        j = int(q[p])
        new = dict(cols[int(q[n - 1])])
        new[p % n] = new.get(p % n, 0) + 2 ** 40 + 1
        f.replace_column(j, list(new), list(new.values()))
        f.run(0)
        cols[j] = new
        again = f.ratio_test(*b, sense=sense, winners=True)
        nAp = np.cumsum([0] + [len(c) for c in cols]).astype(np.int64)
        nAi = np.array([r for c in cols for r in c], np.int32)
        nAlen, nAlimbs = slab([v for c in cols for v in c.values()])
        g = sl.Factorization(n, nAp, nAi, nAlen, nAlimbs, q, lib_path=lib_path, **kw)
        try:
            g.run(0)
            fresh = g.ratio_test(*b, sense=sense, winners=True)
            assert all(np.array_equal(u, v) for u, v in zip(again, fresh))
            if not light:
                check_handle(f, n, handle_problems(n, cols, q, 14)[::2])
            # the other services of the handle afterwards: what they return on a fresh handle, and exact
            xs, xg = f.solve(*rhs), g.solve(*rhs)
            assert np.array_equal(xs[0], xg[0]) and np.array_equal(xs[1], xg[1])
            assert f.check(*rhs, *xs)[0]
            det = oracle_lib.bigints(*f.pivots())[-1]
            same_slab(f.multiply(*xs), [det * v for v in probs[0][0]], "multiply(solve(b))")
        finally:
            g.close()
    finally:
        f.close()


# ---- 8. rejections: SLIP_HIP_INCORRECT_INPUT (-3), nothing written ----

def check_rejections(lib_path, name="gen_n40", **kw):
    import slip_lu_amd as sl
    from slip_lu_amd import _lib
    lib = _lib.load(lib_path)
    xlen, xlimbs = slab([5, -(2 ** 64), 1])
    alen, alimbs = slab([1, 2 ** 64 + 1, -3])
    res = [np.full(2, 77, np.int32) for _ in range(3)]
    R = [r.ctypes.data for r in res]
    X_, A_, NONE = (xlen.ctypes.data, xlimbs.ctypes.data, xlimbs.size), (alen.ctypes.data, alimbs.ctypes.data, alimbs.size), (None, None, 0)
    bad = [(0, 1, *X_, *A_, 1, None, *R, None), (-1, 1, *X_, *A_, 1, None, *R, None),            # n <= 0
           (3, 0, *X_, *A_, 1, None, *R, None),                                                  # nprob < 1
           (3, 1, *X_, *A_, 0, None, *R, None), (3, 1, *X_, *A_, 2, None, *R, None),            # sense
           (3, 1, *X_, None, A_[1], A_[2], 1, None, *R, None), (3, 1, *X_, A_[0], None, A_[2], 1, None, *R, None),      # one of alen / alimbs
           (3, 1, None, X_[1], X_[2], *A_, 1, None, *R, None), (3, 1, X_[0], None, X_[2], *A_, 1, None, *R, None),
           (3, 1, X_[0], X_[1], X_[2] - 1, *A_, 1, None, *R, None),                              # slabs longer than their capacity
           (3, 1, *X_, A_[0], A_[1], A_[2] - 1, 1, None, *R, None),
           (3, 1, X_[0], X_[1], X_[2] - 1, *NONE, 1, None, *R, None),
           (3, 1, *X_, *A_, 1, None, None, R[1], R[2], None), (3, 1, *X_, *A_, 1, None, R[0], None, R[2], None),
           (3, 1, *X_, *A_, 1, None, R[0], R[1], None, None)]                                    # NULL results
    for args in bad:
        assert lib.slip_hip_ratio_test(*args) == -3, args[:2]
    assert all((r == 77).all() for r in res)
    assert lib.slip_hip_ratio_test_paths(None) == -3
    with pytest.raises(ValueError):
        sl.ratio_test(2, xlen, xlimbs, alen, alimbs, lib_path=lib_path)
    got = sl.ratio_test(3, xlen, xlimbs, alen, alimbs, lib_path=lib_path)
    assert [int(v[0]) for v in got] == list(oracle([5, -(2 ** 64), 1], [1, 2 ** 64 + 1, -3], 1))
    # on a handle
    _, fix = load_case(name)
    n, Ap, Ai, Alen, Alimbs, q = len(fix["q"]), fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"]
    b = slab([(-1) ** t * (t % 7) for t in range(2 * n)])
    bl, bv = b[0].ctypes.data, b[1].ctypes.data
    pl, px, nl = C.c_void_p(), C.c_void_p(), C.c_int64()
    outs = (C.byref(pl), C.byref(px), C.byref(nl))
    f = sl.Factorization(n, Ap, Ai, Alen, Alimbs, q, lib_path=lib_path, **kw)
    try:
        f.run(n // 2)
        assert f.info()["K"] < n
        with pytest.raises(sl.SlipError) as e:                    # an incomplete factorisation
            f.ratio_test(*b)
        assert e.value.code == -3
        f.run(0)
        fn = lib.slip_hip_factor_ratio_test
        bad = [(None, 0, 1, bl, bv, 1, None, *R, *outs, None), (f.h, 0, 0, bl, bv, 1, None, *R, *outs, None),
               (f.h, 0, 1, None, bv, 1, None, *R, *outs, None), (f.h, 0, 1, bl, None, 1, None, *R, *outs, None),
               (f.h, 0, 1, bl, bv, 0, None, *R, *outs, None), (f.h, 1, 1, bl, bv, -2, None, *R, *outs, None),
               (f.h, 0, 1, bl, bv, 1, None, None, R[1], R[2], *outs, None), (f.h, 0, 1, bl, bv, 1, None, R[0], None, R[2], *outs, None),
               (f.h, 0, 1, bl, bv, 1, None, R[0], R[1], None, *outs, None),
               (f.h, 0, 1, bl, bv, 1, None, *R, outs[0], None, outs[2], None)]                   # half of the winners' slab
        for args in bad:
            assert fn(*args) == -3, args[1:3]
        assert all((r == 77).all() for r in res) and pl.value is None and px.value is None
        assert lib.slip_hip_factor_ratio_test_paths(f.h, None) == -3 and lib.slip_hip_factor_ratio_test_paths(None, R[0]) == -3
        with pytest.raises(ValueError):
            f.ratio_test(*b, nprob=2)
        with pytest.raises(ValueError):
            f.ratio_test(*b, key=np.zeros(n + 1, np.int32))
        fac = f.download()
        tr = f.ratio_test(*b, transpose=True, winners=True)
    finally:
        f.close()
    g = sl.Factorization.from_factors(fac, lib_path=lib_path, **{k: v for k, v in kw.items() if k in ("waves", "workers")})
    try:
        with pytest.raises(sl.SlipError) as e:                    # a handle around given factors holds no q
            g.ratio_test(*b)
        assert e.value.code == -3
        assert all(np.array_equal(u, v) for u, v in zip(g.ratio_test(*b, transpose=True, winners=True), tr))
    finally:
        g.close()
