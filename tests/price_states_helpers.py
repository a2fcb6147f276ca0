"""Shared by tests/test_emu_price_states.py (the emulator build) and tests/test_gpu_price_states.py (the product on the
device): pricing with nonbasic states and reference weights (slip_hip_factor_price_states fused on a handle,
slip_hip_price_select on caller slabs).  The oracle is Python fractions in the direct formulation: v_j = X_j / det and
alpha_j = A_j / det as true values (on the small goldens from a Gauss-Jordan solve in fractions that shares nothing with the
library), the eligibility rule of every state on their signs, the score |v_j| or v_j^2 / w_j, the ratio v_j / (sense *
alpha_j).  Every comparison is exact equality.  lib_path None is the product library."""
import ctypes as C
import random
from fractions import Fraction

import numpy as np
import pytest

import oracle_lib
from bound_helpers import make_bounds
from check_helpers import columns, slab
from conftest import load_case
from price_helpers import COMBOS, Case, random_columns, shifted, small_costs, small_rhs
from product_helpers import Mat, same_slab
from ratio_helpers import handle_problems, padded_slab

B = 2 ** 32
ONES = lambda digits: B ** digits - 1                              # every digit all ones


def sign(v):
    return (v > 0) - (v < 0)


# ---- the oracle ----

def oracle(vs, als, state, weights, nside, sense, key):
    """(best, nties, neligible, vsign) of one problem from the true values v_j (and alpha_j, nside 2)"""
    ncols = len(vs)
    if nside == 1:
        t = [sense * v for v in vs]
        el = [j for j in range(ncols) if (state[j] == 1 and t[j] < 0) or (state[j] == 2 and t[j] > 0) or (state[j] == 3 and t[j] != 0)]
        score = {j: abs(vs[j]) if weights is None else vs[j] * vs[j] / weights[j] for j in el}
        top = max(score.values()) if el else None
    else:
        t = [sense * a for a in als]                               # sense * s * A_j has the sign of sense * alpha_j
        el = [j for j in range(ncols) if (state[j] == 1 and t[j] > 0) or (state[j] == 2 and t[j] < 0) or (state[j] == 3 and t[j] != 0)]
        score = {j: vs[j] / (sense * als[j]) for j in el}
        top = min(score.values()) if el else None
    if not el:
        return -1, 0, 0, 0
    ties = [j for j in el if score[j] == top]
    best = min(ties, key=lambda j: (int(key[j]) if key is not None else 0, j))
    return best, len(ties), len(el), sign(vs[best])


def eligible_states(vs, als, state, nside, sense):
    """the states of the eligible columns of one problem"""
    out = set()
    for j, st in enumerate(state):
        if oracle([vs[j]], None if als is None else [als[j]], [st], None, nside, sense, None)[0] == 0:
            out.add(st)
    return out


def draw_states(ncols, seed):
    """a state per column, all four present from four columns on"""
    rng = random.Random(seed)
    st = [j % 4 for j in range(ncols)] if ncols >= 4 else [3] * ncols
    rng.shuffle(st)
    return st


def draw_weights(ncols, seed, wide=False):
    rng = random.Random(seed)
    return [rng.randrange(1, 50) if not wide or j % 3 else rng.randrange(B ** 39, B ** 40) for j in range(ncols)]


def fraction_tsolve(n, cols, q, bvecs):
    """y_c with A(:,q)^T y_c = b_c in fractions (b by position, y by row id): Gauss-Jordan, nothing of the library in it"""
    T = [[Fraction(cols[int(q[k])].get(i, 0)) for i in range(n)] + [Fraction(b[k]) for b in bvecs] for k in range(n)]
    for c in range(n):
        p = next(r for r in range(c, n) if T[r][c] != 0)
        T[c], T[p] = T[p], T[c]
        inv = 1 / T[c][c]
        T[c] = [v * inv for v in T[c]]
        for r in range(n):
            if r != c and T[r][c] != 0:
                f = T[r][c]
                T[r] = [a - f * b for a, b in zip(T[r], T[c])]
    return [[T[i][n + c] for i in range(n)] for c in range(len(bvecs))]


def handle_ynum(case, bvecs):
    """the numerators of the handle's own solve_transpose (pinned to the reference elsewhere), one list per vector"""
    n = case.n
    y = oracle_lib.bigints(*case.f.solve_transpose(*slab([v for b in bvecs for v in b]), nrhs=len(bvecs)))
    return [y[c * n:(c + 1) * n] for c in range(len(bvecs))]


def true_values(case, mat, bvecs, nprob, nside, gs, ynum=None):
    """per problem (v, alpha or None) as fractions.  ynum (a golden too large for a solve in fractions): y is handle_ynum's
    numerators over det, one list per vector of bvecs"""
    if ynum is not None:
        ys, den = ynum, case.det                                   # the sums in integers, one fraction per column
    else:
        ys, den = fraction_tsolve(case.n, case.cols, case.q, bvecs), 1
    out = []
    for c in range(nprob):
        yx = ys[nside * c]
        v = [Fraction(sum(a * yx[i] for i, a in col.items()), den) - (gs[c][j] if gs is not None else 0) for j, col in enumerate(mat.last)]
        al = [Fraction(sum(a * ys[2 * c + 1][i] for i, a in col.items()), den) for col in mat.last] if nside == 2 else None
        out.append((v, al))
    return out


def expected(vals, d, state, weights, nside, sense, key):
    """per problem the oracle's four results, and the flat winners X_best, A_best (integers: the true values times d_c)"""
    want, win = [], []
    for c, (v, al) in enumerate(vals):
        dc = d[c] if isinstance(d, (list, tuple)) else d
        w = oracle(v, al, state, weights, nside, sense, key)
        X = v[w[0]] * dc if w[0] >= 0 else Fraction(0)
        A = al[w[0]] * dc if w[0] >= 0 and nside == 2 else Fraction(0)
        assert X.denominator == 1 and A.denominator == 1
        want.append(w)
        win += [int(X), int(A)]
    return want, win


def same_results(got, want, win, what=""):
    nprob = len(want)
    assert [tuple(int(got[t][c]) for t in range(4)) for c in range(nprob)] == want, what
    same_slab(got[4:], win, what)


KEY = lambda ncols: np.array([(7 * j) % 5 for j in range(ncols)], np.int32)


def check_states(case, dev, mat, bvecs, nprob, nside, state, weights=None, gs=None, combos=COMBOS, ynum=None, inspect=None, plain=True):
    """price_states on one set of operands under every combination against the oracle; returns the summed path counts"""
    f, ncols = case.f, mat.ncols
    b = slab([v for bb in bvecs for v in bb])
    cost = slab([v for g in gs for v in g]) if gs is not None else None
    vals = true_values(case, mat, bvecs, nprob, nside, gs, ynum)
    if inspect:
        inspect(vals)
    wt = slab(weights) if weights is not None else None
    total = [0] * 8
    for sense, with_key in combos:
        key = KEY(ncols) if with_key else None
        want, win = expected(vals, case.det, state, weights, nside, sense, key)
        got = f.price_states(dev, *b, state, weights=wt, nprob=nprob, sides=nside, cost=cost, sense=sense, key=key, winners=True)
        same_results(got, want, win, (nside, sense, with_key))
        paths = f.price_states_paths()
        nel = sum(w[2] for w in want)
        assert sum(paths[:4]) == nel and paths[4] == nel and (weights is not None or paths[0] == nel), paths
        ms = f.price_states_ms()
        assert len(ms) == 2 and all(v >= 0 for v in ms)
        if plain:                                                  # without the winners' slab: the same four arrays
            four = f.price_states(dev, *b, state, weights=wt, nprob=nprob, sides=nside, cost=cost, sense=sense, key=key)
            assert len(four) == 4 and all(np.array_equal(u, v) for u, v in zip(four, got[:4]))
        total = [u + v for u, v in zip(total, paths)]
    return total


def select(lib_path, ncols, probs, ds, state, weights=None, nside=1, sense=1, key=None, pad=None, winners=True):
    """slip_hip_price_select on the problems [(X, A or None), ...] over ds"""
    import slip_lu_amd as sl
    x = padded_slab([v for X, _ in probs for v in X], pad)
    a = padded_slab([v for _, A in probs for v in A], pad) if nside == 2 else (None, None)
    return sl.price_select(ncols, *x, *slab(ds), state, alen=a[0], alimbs=a[1], weights=None if weights is None else slab(weights),
                           nprob=len(probs), sides=nside, sense=sense, key=key, winners=winners, lib_path=lib_path)


def check_select(lib_path, ncols, probs, ds, state, weights=None, nside=1, sense=1, key=None, pad=None):
    """price_select against the oracle on v_j = X_j / d_c, alpha_j = A_j / d_c; returns the path counts"""
    import slip_lu_amd as sl
    vals = [([Fraction(x, d) for x in X], [Fraction(a, d) for a in A] if nside == 2 else None) for (X, A), d in zip(probs, ds)]
    want, win = expected(vals, list(ds), state, weights, nside, sense, key)
    got = select(lib_path, ncols, probs, ds, state, weights, nside, sense, key, pad)
    same_results(got, want, win, (nside, sense))
    return sl.price_select_paths(lib_path=lib_path), want


# ---- 1. geometry: the 64-entry rounds of the classify pass and of the selection ----

def check_geometry(lib_path, sizes=(1, 63, 64, 65, 130), shapes=((1, 1), (1, 2), (3, 1), (3, 2)), name="gen_n40", light=False, **kw):
    """(nprob, nside) in shapes on every ncols, the weights on every other nside = 1 shape; light, for the emulator: one
    combination of (sense, key) each, taken in turn"""
    with Case(lib_path, name, **kw) as case:
        n = case.n
        bvecs = small_rhs(n, 6, 21)
        for ncols in sizes:
            mat = Mat(n, ncols, shifted(n, case.cols, ncols))
            state = draw_states(ncols, 100 + ncols)
            assert ncols < 4 or set(state) == {0, 1, 2, 3}
            dev = mat.device(lib_path)
            try:
                for t, (nprob, nside) in enumerate(shapes):
                    combos = COMBOS[(t + ncols) % 4:][:1] if light else COMBOS
                    gs = small_costs(ncols, nprob, 22 + ncols) if nside == 1 else None

                    def together(vals):                            # in some problem, eligible columns of states 1, 2 and 3
                        if ncols >= 63:
                            for sense, _ in combos:
                                assert any(eligible_states(v, al, state, nside, sense) == {1, 2, 3} for v, al in vals), (ncols, nside, sense)

                    check_states(case, dev, mat, bvecs[:nside * nprob], nprob, nside, state,
                                 draw_weights(ncols, 23 + ncols) if nside == 1 and nprob == 3 else None, gs, combos, inspect=together)
            finally:
                dev.close()


# ---- 2. degenerate outcomes ----

def check_degenerate(lib_path, name="test_mat", **kw):
    # nothing is eligible: state 0 everywhere, on a handle and on slabs, with and without weights
    with Case(lib_path, name, **kw) as case:
        n = case.n
        mat = Mat(n, 7, shifted(n, case.cols, 7))
        dev = mat.device(lib_path)
        try:
            for nside, weights in ((1, None), (1, draw_weights(7, 31)), (2, None)):
                got = case.f.price_states(dev, *slab([v for b in small_rhs(n, 2 * nside, 32) for v in b]), [0] * 7,
                                          weights=None if weights is None else slab(weights), nprob=2, sides=nside, winners=True)
                assert all([int(v) for v in got[t]] == [w, w] for t, w in enumerate((-1, 0, 0, 0)))
                assert not got[4].any() and got[5].size == 0
                assert case.f.price_states_paths() == [0] * 8
        finally:
            dev.close()
    got = select(lib_path, 5, [([3, -4, 5, 0, 1], None)], [7], [0] * 5, weights=[1, 2, 3, 4, 5])
    assert [int(g[0]) for g in got[:4]] == [-1, 0, 0, 0] and not got[4].any() and got[5].size == 0
    # every eligible column ties exactly.  Without weights |v_j| = 5/3 (d = -3); with weights v_j^2 / w_j = 1 from DIFFERENT
    # pairs (2, 4), (3, 9), (-4, 16), (1, 1), (-5, 25); column 0 has the wrong sign for its state and column 6 is never eligible
    key = np.array([9, 4, 2, 2, 8, 2, 0], np.int32)
    d = -3
    for sense in (1, -1):
        state = [1, 3, 3, 1, 2, 3, 0]
        v = [sense * 5, -5, 5, -sense * 5, sense * 5, -5, 5]       # thirds: column 0 is at its lower bound with sense * v > 0
        X = [t * d // 3 for t in v]
        for k in (None, key):
            paths, want = check_select(lib_path, 7, [(X, None)], [d], state, None, 1, sense, k)
            assert want[0][:3] == ((2 if k is not None else 1), 5, 5), want
            assert paths[:4] == [5, 0, 0, 0]
        V, W = [2, 3, -4, 1, -5, 7, 2], [4, 9, 16, 1, 25, 49, 4]
        state = [3, 3, 3, 3, 3, 0, 0]
        for k in (None, key):
            paths, want = check_select(lib_path, 7, [([v * d for v in V], None)], [d], state, W, 1, sense, k)
            assert want[0][:3] == ((2 if k is not None else 0), 5, 5), want
            assert paths[:4] == [0, 5, 0, 0]
    # a free column that wins with v_j < 0, another with v_j > 0 (two problems, two signs of d); a zero X_j on a free column
    # is not eligible
    state = [1, 3, 2, 3]
    probs = [([1, -9, 2, 0], None), ([1, -9, 2, 0], None), ([0, 0, 0, 0], None)]
    for weights in (None, [3, 1, 2, 1]):
        paths, want = check_select(lib_path, 4, probs, [4, -4, 1], state, weights, 1, -1)
        assert [w[0] for w in want] == [1, 1, -1] and [w[3] for w in want] == [-1, 1, 0]
        assert want[0][2] == 2 and want[1][2] == 2                 # (column 0 at lower with d > 0, column 2 at upper with d < 0)
    paths, want = check_select(lib_path, 4, [([5, -9, 2, 0], [1, 2, -3, 4]), ([5, 9, 2, 1], [1, 2, -3, 0])], [4, -4], state, None, 2, 1)
    assert [w[0] for w in want] == [1, 1] and [w[3] for w in want] == [-1, -1] and [w[2] for w in want] == [4, 1]


# ---- 3. a negative determinant: eligibility follows v_j, not X_j ----

def check_negative_det(lib_path, name="gen_n40", light=False, **kw):
    with Case(lib_path, name, negative=True, **kw) as case:
        n = case.n
        assert case.det < 0, "det must be negative on this handle"
        ncols = 12 if light else n + 10
        mat = Mat(n, ncols, shifted(n, case.cols, ncols - 4) + random_columns(n, 4, 61))
        state = draw_states(ncols, 62)
        bvecs = small_rhs(n, 4, 63)
        dev = mat.device(lib_path)
        try:
            def differs(vals):                 # columns at a bound with a nonzero value: X_j = det * v_j has the other sign there
                for v, al in vals:
                    assert any(state[j] in (1, 2) and (v if al is None else al)[j] != 0 for j in range(ncols))
            for nside, weights in ((1, None), (1, draw_weights(ncols, 64)), (2, None)):
                check_states(case, dev, mat, bvecs[:2 * nside], 2, nside, state, weights, small_costs(ncols, 2, 65) if nside == 1 else None,
                             COMBOS[1:3] if light else COMBOS, inspect=differs)
        finally:
            dev.close()
        return case.det


# ---- 4. against the existing calls ----

def check_against_price(lib_path, name="gen_n40", **kw):
    import slip_lu_amd as sl
    with Case(lib_path, name, **kw) as case:
        n, f, det = case.n, case.f, case.det
        ncols = 20
        mat = Mat(n, ncols, shifted(n, case.cols, 14) + random_columns(n, 6, 71))
        gs = small_costs(ncols, 2, 72)
        cost = slab([v for g in gs for v in g])
        ones = [1] * ncols
        key = KEY(ncols)
        dev = mat.device(lib_path)
        try:
            # nside 2, every column at its lower bound: slip_hip_factor_price word for word
            bvecs = small_rhs(n, 4, 73)
            b = slab([v for bb in bvecs for v in bb])
            for sense, k in ((1, None), (-1, key)):
                old = f.price(dev, *b, nprob=2, sides=2, sense=sense, key=k, winners=True)
                new = f.price_states(dev, *b, ones, nprob=2, sides=2, sense=sense, key=k, winners=True)
                assert all(np.array_equal(u, v) for u, v in zip(old, new)), sense
            # nside 1, at lower, no weights: price's answer whenever the smallest sense * v_j is negative
            b1 = slab([v for bb in bvecs[:2] for v in bb])
            seen = 0
            for sense, k in ((1, None), (-1, key), (1, key), (-1, None)):
                old = f.price(dev, *b1, nprob=2, sides=1, cost=cost, sense=sense, key=k, winners=True)
                new = f.price_states(dev, *b1, ones, nprob=2, sides=1, cost=cost, sense=sense, key=k, winners=True)
                for c in range(2):
                    if int(old[3][c]) * sense < 0:
                        seen += 1
                        assert all(int(old[t][c]) == int(new[t][c]) for t in (0, 1, 3)), (sense, c)
                        assert np.array_equal(old[4][2 * c:2 * c + 2], new[4][2 * c:2 * c + 2])
                if all(int(v) * sense < 0 for v in old[3]):
                    assert np.array_equal(old[5], new[5])
            assert seen >= 2
            # price_select on the slabs the three-call route returns: the fused call
            state = draw_states(ncols, 74)
            for nside, weights in ((1, None), (1, draw_weights(ncols, 75, wide=True)), (2, None)):
                bb = slab([v for x in bvecs[:2 * nside] for v in x])
                y = f.solve_transpose(*bb, nrhs=2 * nside)
                r = oracle_lib.bigints(*dev.multiply(*y, nvec=2 * nside, transpose=True))
                X = slab([v for c in range(2) for v in r[nside * c * ncols:(nside * c + 1) * ncols]])
                A = slab([v for c in range(2) for v in r[(2 * c + 1) * ncols:(2 * c + 2) * ncols]]) if nside == 2 else (None, None)
                wt = None if weights is None else slab(weights)
                fused = f.price_states(dev, *bb, state, weights=wt, nprob=2, sides=nside, sense=-1, key=key, winners=True)
                loose = sl.price_select(ncols, *X, *slab([det, det]), state, alen=A[0], alimbs=A[1], weights=wt, nprob=2, sides=nside,
                                        sense=-1, key=key, winners=True, lib_path=lib_path)
                assert all(np.array_equal(u, v) for u, v in zip(fused, loose)), nside
                assert f.price_states_paths() == sl.price_select_paths(lib_path=lib_path)
        finally:
            dev.close()


# ---- 5. width classes of the squares, handle-less, six columns ----

# |X_j| by class: (operands, the expected [no product, lane, registers, memory] with every column eligible)
WIDTH_CLASSES = (
    # one and two digits: squared in a lane
    ([1, ONES(1), B, ONES(2), 2 ** 63, 3], [0, 6, 0, 0]),
    # three digits, the first register entry; D = 1 | 2 by BIT length: a square of exactly 64 * 32 bits (32 digits, all ones)
    # and one bit more (2^1024: 33 digits); odd digit counts
    ([B ** 2, ONES(3), ONES(32), B ** 32, ONES(5) - 77, ONES(31)], [0, 0, 6, 0]),
    # D = 2 | 3 at 128 digits, D = 3 | 4 at 192
    ([ONES(64), B ** 64, ONES(96), B ** 96, ONES(63), ONES(65)], [0, 0, 6, 0]),
    # D = 4 | memory at 256 digits: 128 digits all ones square to exactly 256 * 32 bits; 2^4096 (129 digits) is one bit more
    ([ONES(128), B ** 128, ONES(127), ONES(129), ONES(300), B ** 299 + 12345], [0, 0, 2, 4]),
    # a mixture, one column of each path and a zero
    ([7, ONES(2) - 5, ONES(40), ONES(130), 0, B ** 128 - B ** 3], [0, 2, 2, 1]),
)


def check_width_classes(lib_path):
    """No operand has 2 * dig(X) = 258 digits and a square within 256 * 32 bits: dig(X) = 129 means |X| >= 2^4096 and a square
    of at least 8193 bits, so the bit-length rule and the digit rule part only between 2 dig(X) - 1 and 2 dig(X), never across
    a class edge (all four edges are even).  Both sides of every edge are here by their exact bit lengths instead."""
    rng = random.Random(81)
    for t, (mags, paths_want) in enumerate(WIDTH_CLASSES):
        X = [m if j % 2 else -m for j, m in enumerate(mags)]
        # weights of one digit and of forty digits; high zero limbs on some entries; state 3 with a nonzero X_j is always eligible
        for weights in ([rng.randrange(1, B) for _ in range(6)], [rng.randrange(B ** 39, B ** 40) for _ in range(6)]):
            for d, pad in ((5, None), (-(B ** 3) - 1, [0, 2, 1, 0, 3, 1] * 2)):
                probs = [(X, None), ([-x for x in reversed(X)], None)]
                want_paths = [2 * p for p in paths_want]
                paths, want = check_select(lib_path, 6, probs, [d, -d], [3] * 6, weights, 1, 1 if t % 2 else -1, None, pad)
                assert paths[:4] == want_paths, (t, paths)
                assert paths[4] == sum(want_paths) == sum(w[2] for w in want)
    # the same operands without weights: no product at all
    X = [m * (-1) ** j for j, m in enumerate(WIDTH_CLASSES[3][0])]
    paths, _ = check_select(lib_path, 6, [(X, None)], [-1], [3, 1, 2, 3, 1, 2], None, 1, -1)
    assert paths[0] > 0 and paths[1:4] == [0, 0, 0]


def check_natural_wide(lib_path, name="de080285"):
    """a golden whose X_j are hundreds of limbs wide: Dantzig with states, weights of one digit and of det's size, the dual
    ratio test; the squares go through memory"""
    with Case(lib_path, name) as case:
        n = case.n
        mat = Mat(n, 40, shifted(n, case.cols, 30) + random_columns(n, 10, 51))
        probs = handle_problems(n, case.cols, case.q, 52)[::2]
        bvecs = [side for pr in probs for side in pr]
        state = draw_states(40, 53)
        rng = random.Random(54)
        big = [abs(case.det) + rng.randrange(1, B) for _ in range(40)]
        dev = mat.device(lib_path)
        try:
            ynum = handle_ynum(case, bvecs)
            one = dict(combos=((-1, True),), ynum=ynum[::2], plain=False)
            check_states(case, dev, mat, bvecs[::2], 2, 1, state, None, None, **one)
            p1 = check_states(case, dev, mat, bvecs[::2], 2, 1, state, draw_weights(40, 55), None, **one)
            p2 = check_states(case, dev, mat, bvecs[::2], 2, 1, state, big, None, **one)
            assert p1[3] > 0 and p2[3] > 0, "the memory path of the squares was not reached"
            check_states(case, dev, mat, bvecs, 2, 2, state, None, None, ((1, True),), ynum=ynum, plain=False)
        finally:
            dev.close()


# ---- 6. grouping ----

def check_groups(lib_path, monkeypatch, name="gen_n40", **kw):
    """a staging bound below one problem's need: every problem is its own group, of the products and of the squares; the
    results are those of the ungrouped call"""
    with Case(lib_path, name, **kw) as case:
        n = case.n
        mat = Mat(n, 20, shifted(n, case.cols, 14) + random_columns(n, 6, 71))
        gs = small_costs(20, 3, 72)
        state, weights = draw_states(20, 73), draw_weights(20, 74, wide=True)
        dev = mat.device(lib_path)
        try:
            for nside, wts in ((1, weights), (2, None)):
                bvecs = small_rhs(n, 3 * nside, 75)
                b, cost = slab([v for bb in bvecs for v in bb]), slab([v for g in gs for v in g]) if nside == 1 else None
                args = dict(weights=None if wts is None else slab(wts), nprob=3, sides=nside, cost=cost, sense=-1, winners=True)
                whole = case.f.price_states(dev, *b, state, **args)
                monkeypatch.setenv("SLIP_HIP_PRODUCT_STAGE_KB", "1")
                parts = case.f.price_states(dev, *b, state, **args)
                assert all(np.array_equal(u, v) for u, v in zip(whole, parts))
                check_states(case, dev, mat, bvecs, 3, nside, state, wts, gs if nside == 1 else None, ((-1, True),))
                monkeypatch.delenv("SLIP_HIP_PRODUCT_STAGE_KB")
        finally:
            dev.close()
    # the squares' own groups, on slabs: three problems of wide operands under a bound of 1 KiB
    X = [ONES(40) - j for j in range(6)]
    probs = [(X, None), ([-x for x in X], None), (X[::-1], None)]
    whole = select(lib_path, 6, probs, [3, 3, -3], [3] * 6, [5, 4, 3, 2, 1, 6])
    monkeypatch.setenv("SLIP_HIP_PRODUCT_STAGE_KB", "1")
    parts = select(lib_path, 6, probs, [3, 3, -3], [3] * 6, [5, 4, 3, 2, 1, 6])
    assert all(np.array_equal(u, v) for u, v in zip(whole, parts))
    check_select(lib_path, 6, probs, [3, 3, -3], [3] * 6, [5, 4, 3, 2, 1, 6])
    monkeypatch.delenv("SLIP_HIP_PRODUCT_STAGE_KB")


# ---- 7. lifecycle ----

def check_lifecycle(lib_path, name="gen_n40", **kw):
    import slip_lu_amd as sl
    with Case(lib_path, name, **kw) as case:
        n, f, q = case.n, case.f, case.q
        mat = Mat(n, 12, shifted(n, case.cols, 8) + random_columns(n, 4, 81))
        bvecs = small_rhs(n, 2, 82)
        b, rhs = slab([v for bb in bvecs for v in bb]), slab(bvecs[0])
        state, wt = draw_states(12, 83), slab(draw_weights(12, 84))
        yv = slab([(-1) ** t * (t + 2 ** (5 * t)) for t in range(n)])
        bnd = make_bounds(n, {"kind": [(t % 3) + 1 for t in range(n)], "lo": [-t for t in range(n)], "hi": [t + 1 for t in range(n)], "den": 1})
        dev = mat.device(lib_path)
        try:
            def older():
                return (f.solve(*rhs), f.solve_transpose(*rhs), dev.multiply(*yv, transpose=True), f.ratio_test(*b, winners=True),
                        f.price(dev, *b, sides=2, winners=True), f.ratio_test_bounded(*b, bnd, winners=True),
                        f.bound_test(*rhs, bnd, winners=True))

            before = older()
            first = f.price_states(dev, *b, state, sides=2, winners=True)
            again = f.price_states(dev, *b, state, sides=2, winners=True)             # twice in a row: identical
            assert all(np.array_equal(u, v) for u, v in zip(first, again))
            weighted = f.price_states(dev, *rhs, state, weights=wt, sides=1, sense=-1, winners=True)
            for u, v in zip(before, older()):
                assert len(u) == len(v) and all(np.array_equal(s, t) for s, t in zip(u, v))
            check_states(case, dev, mat, bvecs, 1, 2, state, None, None, ((1, False),))
            # a column replaced and factorised again: the answer for the NEW matrix, as a fresh handle gives it
            cols = [dict(c) for c in case.cols]
            j = int(q[n // 2])
            new = dict(cols[int(q[n - 1])])
            new[j % n] = new.get(j % n, 0) + 2 ** 40 + 1
            f.replace_column(j, list(new), list(new.values()))
            f.run(0)
            cols[j] = new
            replaced = (f.price_states(dev, *b, state, sides=2, winners=True),
                        f.price_states(dev, *rhs, state, weights=wt, sides=1, sense=-1, winners=True))
            nAp = np.cumsum([0] + [len(c) for c in cols]).astype(np.int64)
            nAi = np.array([r for c in cols for r in c], np.int32)
            nAlen, nAlimbs = slab([v for c in cols for v in c.values()])
            h = sl.Factorization(n, nAp, nAi, nAlen, nAlimbs, q, lib_path=lib_path, **kw)
            try:
                h.run(0)
                fresh = (h.price_states(dev, *b, state, sides=2, winners=True),
                         h.price_states(dev, *rhs, state, weights=wt, sides=1, sense=-1, winners=True))
                assert all(np.array_equal(u, v) for r, s in zip(replaced, fresh) for u, v in zip(r, s))
            finally:
                h.close()
            assert len(weighted) == 6
        finally:
            dev.close()


# ---- 8. rejections: SLIP_HIP_INCORRECT_INPUT (-3), nothing written ----

def check_rejections(lib_path, name="test_mat", **kw):
    import slip_lu_amd as sl
    from slip_lu_amd import _lib
    lib = _lib.load(lib_path)
    _, fix = load_case(name)
    n, Ap, Ai, Alen, Alimbs, q = len(fix["q"]), fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"]
    cols = columns(n, Ap, Ai, oracle_lib.bigints(Alen, Alimbs))
    mat, other = Mat(n, 5, shifted(n, cols, 5)), Mat(n + 1, 5, shifted(n, cols, 5))
    b = slab([(-1) ** t * (t % 7) for t in range(2 * n)])
    glen, glimbs = slab([3, -(2 ** 64), 0, 1, 2 ** 70])
    res = [np.full(2, 77, np.int32) for _ in range(4)]
    R = [r.ctypes.data for r in res]
    bl, bv, G = b[0].ctypes.data, b[1].ctypes.data, (glen.ctypes.data, glimbs.ctypes.data, glimbs.size)
    pl, px, nl = C.c_void_p(), C.c_void_p(), C.c_int64()
    outs, none = (C.byref(pl), C.byref(px), C.byref(nl)), (None, None, None)
    st = np.array([1, 2, 3, 0, 3], np.int32)
    st4, stm = np.array([1, 2, 4, 0, 3], np.int32), np.array([1, -1, 3, 0, 3], np.int32)
    wl, wv = slab([3, 2 ** 64, 1, 5, 2 ** 70])
    wneg, wzero = slab([3, 2 ** 64, -1, 5, 2 ** 70]), slab([3, 2 ** 64, 1, 0, 2 ** 70])
    wpad = (np.array([1, 2, 1, 2, 2], np.int32), np.array([3, 0, 1, 1, 0, 0, 5, 1], np.uint64))     # entry 3 (state 0): all-zero limbs
    S = (st.ctypes.data, None, None, 0)
    W = lambda s, w, cap=None: (s.ctypes.data, w[0].ctypes.data, w[1].ctypes.data, w[1].size if cap is None else cap)
    f = sl.Factorization(n, Ap, Ai, Alen, Alimbs, q, lib_path=lib_path, **kw)
    dev, wrong = mat.device(lib_path), other.device(lib_path)
    fn = lib.slip_hip_factor_price_states
    try:
        f.run(n // 2)
        assert f.info()["K"] < n
        assert fn(f.h, dev.h, 1, 1, bl, bv, *G, *S, 1, None, *R, *outs, None) == -3            # a run to K < n
        with pytest.raises(sl.SlipError) as e:
            f.price_states(dev, *b, st, sides=2)
        assert e.value.code == -3
        f.run(0)
        head = (f.h, dev.h, 1, 1, bl, bv, *G)
        bad = [(*head, None, None, None, 0, 1, None, *R, *outs, None),                         # a NULL state
               (*head, *W(st4, (wl, wv))[:1], None, None, 0, 1, None, *R, *outs, None),        # a state outside 0..3
               (*head, *W(stm, (wl, wv))[:1], None, None, 0, 1, None, *R, *outs, None),
               (*head, st.ctypes.data, wl.ctypes.data, None, wv.size, 1, None, *R, *outs, None),       # one of wlen / wlimbs
               (*head, st.ctypes.data, None, wv.ctypes.data, wv.size, 1, None, *R, *outs, None),
               (*head, *W(st, (wl, wv), wv.size - 1), 1, None, *R, *outs, None),               # the weights longer than w_limbs
               (*head, *W(st, wneg), 1, None, *R, *outs, None), (*head, *W(st, wzero), 1, None, *R, *outs, None),      # w_j <= 0
               (*head, *W(st, wpad), 1, None, *R, *outs, None),                                # ... as all-zero limbs, on a state 0
               (f.h, dev.h, 2, 1, bl, bv, None, None, 0, *W(st, (wl, wv)), 1, None, *R, *outs, None),  # weights with nside 2
               (*head, *S, 1, None, *R, outs[0], None, outs[2], None), (*head, *S, 1, None, *R, None, outs[1], outs[2], None),
               (*head, *S, 1, None, *R, outs[0], outs[1], None, None), (*head, *S, 1, None, *R, None, None, outs[2], None),
               # everything slip_hip_factor_price refuses
               (None, dev.h, 1, 1, bl, bv, *G, *S, 1, None, *R, *outs, None), (f.h, None, 1, 1, bl, bv, *G, *S, 1, None, *R, *outs, None),
               (f.h, dev.h, 1, 1, None, bv, *G, *S, 1, None, *R, *outs, None), (f.h, dev.h, 1, 1, bl, None, *G, *S, 1, None, *R, *outs, None),
               (f.h, wrong.h, 1, 1, bl, bv, None, None, 0, *S, 1, None, *R, *outs, None),
               (f.h, dev.h, 0, 1, bl, bv, *G, *S, 1, None, *R, *outs, None), (f.h, dev.h, 3, 1, bl, bv, *G, *S, 1, None, *R, *outs, None),
               (f.h, dev.h, 2, 0, bl, bv, *G, *S, 1, None, *R, *outs, None), (f.h, dev.h, 1, -1, bl, bv, *G, *S, 1, None, *R, *outs, None),
               (*head, *S, 0, None, *R, *outs, None), (*head, *S, 2, None, *R, *outs, None),
               (f.h, dev.h, 1, 1, bl, bv, None, G[1], G[2], *S, 1, None, *R, *outs, None),
               (f.h, dev.h, 1, 1, bl, bv, G[0], None, G[2], *S, 1, None, *R, *outs, None),
               (f.h, dev.h, 1, 1, bl, bv, G[0], G[1], G[2] - 1, *S, 1, None, *R, *outs, None)]
        bad += [(*head, *S, 1, None, *[None if t == k else r for t, r in enumerate(R)], *outs, None) for k in range(4)]
        for t, args in enumerate(bad):
            assert fn(*args) == -3, t
        # the handle-less form: x of 5 entries over d
        X, A, D, Z = slab([4, -5, 6, 0, 2 ** 70]), slab([1, -1, 0, 2, 3]), slab([-7]), (np.zeros(1, np.int32), np.zeros(1, np.uint64))
        Dz = (np.array([2], np.int32), np.zeros(2, np.uint64))                                  # a zero d as all-zero limbs
        P = lambda s: (s[0].ctypes.data, s[1].ctypes.data, s[1].size)
        NOA = (None, None, 0)
        sel = lib.slip_hip_price_select
        tail = (1, None, *R, *outs, None)
        badsel = [(5, 1, 1, *P(X), *NOA, *P(D), None, None, None, 0, *tail), (5, 1, 1, *P(X), *NOA, *P(D), *W(st4, (wl, wv))[:1], None, None, 0, *tail),
                  (5, 1, 1, *P(X), *NOA, *P(D), st.ctypes.data, wl.ctypes.data, None, wv.size, *tail),
                  (5, 1, 1, *P(X), *NOA, *P(D), st.ctypes.data, None, wv.ctypes.data, wv.size, *tail),
                  (5, 1, 1, *P(X), *NOA, *P(D), *W(st, (wl, wv), wv.size - 1), *tail),
                  (5, 1, 1, *P(X), *NOA, *P(D), *W(st, wneg), *tail), (5, 1, 1, *P(X), *NOA, *P(D), *W(st, wzero), *tail),
                  (5, 1, 1, *P(X), *NOA, *P(D), *W(st, wpad), *tail),
                  (5, 1, 2, *P(X), *P(A), *P(D), *W(st, (wl, wv)), *tail),                      # weights with nside 2
                  (5, 1, 1, *P(X), *NOA, *P(Z), *S, *tail), (5, 1, 1, *P(X), *NOA, *P(Dz), *S, *tail),  # a zero d_c
                  (5, 1, 2, *P(X), *NOA, *P(D), *S, *tail), (5, 1, 1, *P(X), *P(A), *P(D), *S, *tail),  # a missing / given against nside
                  (5, 1, 1, *P(X), *NOA, *P(D), *S, 1, None, *R, outs[0], None, outs[2], None),
                  (5, 1, 1, *P(X), *NOA, *P(D), *S, 1, None, *R, None, None, outs[2], None),
                  (0, 1, 1, *P(X), *NOA, *P(D), *S, *tail), (5, 0, 1, *P(X), *NOA, *P(D), *S, *tail), (5, 1, 3, *P(X), *NOA, *P(D), *S, *tail),
                  (5, 1, 1, *P(X), *NOA, *P(D), *S, 0, None, *R, *outs, None),
                  (5, 1, 1, None, X[1].ctypes.data, X[1].size, *NOA, *P(D), *S, *tail), (5, 1, 1, *P(X), *NOA, None, D[1].ctypes.data, 1, *S, *tail),
                  (5, 1, 1, *P(X)[:2], X[1].size - 1, *NOA, *P(D), *S, *tail),                  # x longer than x_limbs
                  (5, 1, 2, *P(X), *P(A)[:2], A[1].size - 1, *P(D), *S, *tail)]
        badsel += [(5, 1, 1, *P(X), *NOA, *P(D), *S, 1, None, *[None if t == k else r for t, r in enumerate(R)], *outs, None) for k in range(4)]
        for t, args in enumerate(badsel):
            assert sel(*args) == -3, t
        assert all((r == 77).all() for r in res) and pl.value is None and px.value is None and nl.value == 0
        for fnp in (lib.slip_hip_factor_price_states_ms, lib.slip_hip_factor_price_states_paths):
            assert fnp(f.h, None) == -3 and fnp(None, R[0]) == -3
        assert lib.slip_hip_price_select_paths(None) == -3
        with pytest.raises(ValueError):
            f.price_states(dev, *b, st[:4], sides=2)
        with pytest.raises(ValueError):
            f.price_states(dev, *b, st, weights=slab([1, 2, 3]), nprob=2)
        with pytest.raises(ValueError):
            f.price_states(dev, *b, st, sides=2, key=np.zeros(6, np.int32))
        with pytest.raises(ValueError):
            sl.price_select(5, *X, *D, st[:3], lib_path=lib_path)
        # the same arguments, accepted
        assert fn(*head, *W(st, (wl, wv)), 1, None, *R, *none, None) == 0
        assert all(r[0] != 77 and r[1] == 77 for r in res)
        for r in res:
            r[:] = 77
        assert sel(5, 1, 1, *P(X), *NOA, *P(D), *W(st, (wl, wv)), 1, None, *R, *none, None) == 0
        assert all(r[0] != 77 and r[1] == 77 for r in res)
    finally:
        f.close()
        dev.close()
        wrong.close()


# ---- 9. the ABI ----

def check_abi():
    from slip_lu_amd import _lib
    import slip_lu_amd as sl
    names = ("slip_hip_factor_price_states", "slip_hip_price_select", "slip_hip_factor_price_states_ms",
             "slip_hip_factor_price_states_paths", "slip_hip_price_select_paths")
    assert all(name in _lib.EXPORTS for name in names)
    assert callable(sl.price_select) and callable(sl.price_select_paths)
    assert all(hasattr(sl.Factorization, m) for m in ("price_states", "price_states_ms", "price_states_paths"))
    return names
