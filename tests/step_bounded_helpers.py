"""Shared by tests/test_emu_step_bounded.py (the emulator build) and tests/test_gpu_step_bounded.py (the product on the device):
the bounded exact simplex step (slip_hip_step_bounded on caller slabs, slip_hip_factor_step_bounded fused with a solve on a
handle).  The oracle is Python integers and fractions in the direct formulation on the true values: the step is the minimum
over the entries of (x_i - l_i) / (sense alpha_i) or (u_i - x_i) / (-sense alpha_i), compared with the entering variable's
range er / den, and the new iterate is x - sense theta alpha -- not the transformed formulas of the header.  Every comparison
is exact; a pivot and a flip are also proved end to end against the handle's own solves.  lib_path None is the product library."""
import ctypes as C
import random
from fractions import Fraction

import numpy as np
import pytest

import oracle_lib
from bound_helpers import make_bounds, oracle_steps, pick, winner_ratio
from check_helpers import slab
from pivot_update_helpers import case_handle, handle_problems, one_problem_per_group, with_bits
from product_helpers import same_slab
from ratio_helpers import padded_slab


def digits(v):
    return (abs(v).bit_length() + 31) // 32


# ---- the oracle ----

def oracle_move(xs, avs, d, bnd, sense, key, fin, er, ev):
    """one problem on its true values.  Returns a dictionary: sel = (best, nties, neligible, side), move, tie (the step equals
    the range), value = the entering variable's new value, x = the new basic values (None: unbounded)"""
    el = oracle_steps(xs, avs, d, bnd, sense)
    sel, _ = pick(el, key)
    best, den = sel[0], bnd["den"]
    theta = el[best][0] if best >= 0 else None
    rng = Fraction(er, den) if fin else None
    if fin and (best < 0 or rng <= theta):
        move, t = 2, rng
    elif best >= 0:
        move, t = 1, theta
    else:
        return dict(sel=sel, move=0, tie=False, value=None, x=None)
    x = [Fraction(v, d) - sense * t * Fraction(a, d) for v, a in zip(xs, avs)]
    if move == 1:                                          # the leaving variable sits on the bound `side` names
        assert x[best] == Fraction(bnd["lo" if sel[3] < 0 else "hi"][best], den)
    return dict(sel=sel, move=move, tie=bool(fin and best >= 0 and rng == theta), value=Fraction(ev, den) + sense * t, x=x)


def job_path(X, Y, Z, W):
    """the path of the scalar +-X Y +- Z W, as the header defines it: 0 both terms zero, 1 a lane (both products of at most
    four digits by the factors' digit counts), 2 registers (max(bits) + 1 fits 256 digits), 3 memory"""
    s1, s2 = bool(X and Y), bool(Z and W)
    if not s1 and not s2:
        return 0
    b1 = abs(X).bit_length() + abs(Y).bit_length() if s1 else 0
    b2 = abs(Z).bit_length() + abs(W).bit_length() if s2 else 0
    w1, w2 = (digits(X) + digits(Y) if s1 else 0), (digits(Z) + digits(W) if s2 else 0)
    if w1 <= 4 and w2 <= 4:
        return 1
    return 2 if (max(b1, b2) + 1 + 31) // 32 <= 256 else 3


def scalar_paths(move, fin, best, N, ap, d, den, er, ev):
    """the scalars the new kernel forms for one problem, by path: the comparison (finite and a winner), then the two of the move"""
    out = [0, 0, 0, 0]
    jobs = [(er, ap, N, 1)] if fin and best >= 0 else []
    if move == 1:
        jobs += [(den, ap, 0, 0), (ev, ap, N, 1)]
    if move == 2:
        jobs += [(den, d, 0, 0), (ev, d, er, d)]
    for j in jobs:
        out[job_path(*j)] += 1
    return out


def expected(probs, bnd, ent, sense, key):
    """the whole call: (the selection's four arrays, move, ninexact, R, Dn, E as integers, the oracle's records, the scalars by path)"""
    n, den = len(probs[0][0]), bnd["den"]
    sel, move, nin, R, Dn, E, recs, paths = [], [], [], [], [], [], [], [0, 0, 0, 0]
    for (xs, avs, d), (fin, er, ev) in zip(probs, ent):
        o = oracle_move(xs, avs, d, bnd, sense, key, fin, er, ev)
        recs.append(o); sel.append(o["sel"]); move.append(o["move"])
        best, side = o["sel"][0], o["sel"][3]
        N, ap = winner_ratio(xs, avs, d, bnd, best, side)
        for k, v in enumerate(scalar_paths(o["move"], fin, best, N, ap, d, den, er if fin else 0, ev)):
            paths[k] += v
        if o["move"] == 0:
            R += [0] * n; Dn.append(0); E.append(0); nin.append(0)
            continue
        dn = den * ap if o["move"] == 1 else den * d          # the denominator the header names; everything else follows from the oracle
        e = o["value"] * dn
        assert e.denominator == 1
        bad = 0
        for i, v in enumerate(o["x"]):
            r = v * dn
            if o["move"] == 1 and i == best:
                R.append(int(e))
            elif r.denominator == 1:
                R.append(int(r))
            else:
                R.append(0); bad += 1
        Dn.append(dn); E.append(int(e)); nin.append(bad)
    return sel, move, nin, R, Dn, E, recs, paths


def make_entering(nprob, ent, pad=False):
    import slip_lu_amd as sl
    if ent is None:
        return None
    pads = [1 + c % 2 for c in range(nprob)] if pad else None
    fin = np.array([f for f, _, _ in ent], np.int32)
    er = padded_slab([e if f else 0 for f, e, _ in ent], pads)
    ev = padded_slab([v for _, _, v in ent], pads)
    return sl.Entering(nprob, fin if fin.any() else None, er if fin.any() else None, ev if any(v for _, _, v in ent) else None)


def run(lib_path, probs, bnd, ent=None, sense=1, key=None, pad=False):
    """one call of slip_hip_step_bounded on [(xs, avs, d), ...] with ent = [(finite, er, ev), ...] (None: no entering data)
    against the oracle; returns (the result, the path counts, the oracle's records)"""
    import slip_lu_amd as sl
    n, nprob = len(probs[0][0]), len(probs)
    pads = [t % 3 for t in range(n * nprob)] if pad else None
    x = padded_slab([v for p in probs for v in p[0]], pads)
    a = padded_slab([v for p in probs for v in p[1]], pads)
    d = padded_slab([p[2] for p in probs], [1 + c % 2 for c in range(nprob)] if pad else None)
    res = sl.step_bounded(n, *x, *a, *d, make_bounds(n, bnd, pad), make_entering(nprob, ent, pad), nprob=nprob, sense=sense, key=key,
                          lib_path=lib_path)
    sel, move, nin, R, Dn, E, recs, spaths = expected(probs, bnd, ent or [(0, 0, 0)] * nprob, sense, key)
    for t, (what, got) in enumerate((("best", res.best), ("nties", res.nties), ("neligible", res.neligible), ("side", res.side))):
        assert [int(v) for v in got] == [s[t] for s in sel], (what, sense)
    assert [int(v) for v in res.move] == move, ("move", sense)
    same_slab(res.d, Dn, "the new denominators")
    same_slab(res.e, E, "the entering variables")
    same_slab(res.x, R, "the new numerators")
    assert [int(v) for v in res.ninexact] == nin, "ninexact"
    paths = sl.step_bounded_paths(lib_path=lib_path)
    assert sum(paths[8:12]) == n * nprob and paths[12] == sum(nin), paths
    assert paths[13:16] == [move.count(0), move.count(1), move.count(2)], paths
    assert paths[16:20] == spaths, (paths[16:20], spaths)
    assert all(v >= 0 for v in sl.step_bounded_ms(lib_path=lib_path))
    return res, paths, recs


def same_result(u, v):
    return all(np.array_equal(p, q) for p, q in zip((u.best, u.nties, u.neligible, u.side, u.move, u.ninexact, *u.x, *u.d, *u.e),
                                                    (v.best, v.nties, v.neligible, v.side, v.move, v.ninexact, *v.x, *v.d, *v.e)))


# ---- 1. the three moves ----

def moves_case(rng, n, d, den, sense, flavour):
    """three problems over one set of bounds: [0] a pivot on random data, x inside and outside its bounds, a finite range that
    does not block on every second case; [1] a flip by flavour: 0 an exact tie of the step and the range, 1 er = 0, 2 a finite
    range and nothing eligible, 3 a range below the step; [2] unbounded (nothing eligible, no finite range)"""
    s = 1 if d > 0 else -1
    kind = [rng.choice((1, 2, 3, 3)) for _ in range(n)]
    mid = [rng.randrange(-20, 21) for _ in range(n)]
    lo = [den * (m - rng.randrange(3, 9)) + rng.randrange(den) for m in mid]
    hi = [den * (m + rng.randrange(3, 9)) - rng.randrange(den) for m in mid]
    bnd = dict(kind=kind, lo=lo, hi=hi, den=den)
    ad = abs(d)
    # [0]: numerators over d of values around the box, some outside it
    x0 = [d * m + rng.randrange(-12 * ad, 12 * ad + 1) for m in mid]
    a0 = [rng.randrange(-2 * ad, 2 * ad + 1) for _ in range(n)]
    a0[rng.randrange(n)] = sense * s * (ad + 1)            # (someone is eligible: kind has a bit of either side... or not, n = 1)
    # [1]: inside the box, |alpha_i| <= 1, so that every step is at least 3 -- but for entry j, whose step is exactly 1
    x1 = [d * m for m in mid]
    a1 = [rng.randrange(-ad, ad + 1) for _ in range(n)]
    j = rng.randrange(n)
    if flavour == 2:
        a1 = [0] * n
    else:
        up = rng.random() < 0.5
        kind[j] |= 2 if up else 1
        a1[j] = -sense * d if up else sense * d            # sense alpha_j = -1 / +1
        if up:
            hi[j] = den * (mid[j] + 1)
        else:
            lo[j] = den * (mid[j] - 1)
    x2, a2 = [d * m + 1 for m in mid], [0] * n
    er1 = {0: den, 1: 0, 2: 7, 3: den - 1 if den > 1 else 0}[flavour]
    big = 10 ** 9
    ent = [(rng.randrange(2), big, rng.randrange(-9, 10)), (1, er1, rng.randrange(-9, 10)), (0, 0, rng.randrange(-9, 10))]
    return [(x0, a0, d), (x1, a1, d), (x2, a2, d)], bnd, ent


def check_moves(lib_path, sizes=(1, 63, 64, 65, 130)):
    rng = random.Random(11)
    seen = dict(moves=set(), tie=0, upper=0, lower=0, outside=0, er0=0, nowinner_flip=0)
    t = 0
    for n in sizes:
        for d, den, sense in ((35, 1, 1), (-35, 6, 1), (2 ** 40 + 15, 6, -1), (-(2 ** 70) - 3, 1, -1)):
            probs, bnd, ent = moves_case(rng, n, d, den, sense, t % 4)
            key = np.array([(5 * i) % 3 for i in range(n)], np.int32) if t % 2 else None
            _, _, recs = run(lib_path, probs, bnd, ent, sense, key, pad=t % 3 == 0)
            for o, (fin, er, _) in zip(recs, ent):
                seen["moves"].add(o["move"])
                seen["tie"] += o["tie"]
                seen["upper"] += o["move"] == 1 and o["sel"][3] > 0
                seen["lower"] += o["move"] == 1 and o["sel"][3] < 0
                seen["er0"] += o["move"] == 2 and fin and er == 0
                seen["nowinner_flip"] += o["move"] == 2 and o["sel"][0] < 0
            el = oracle_steps(*probs[0][:2], probs[0][2], bnd, sense)
            seen["outside"] += any(v < 0 for v, _ in el.values())
            assert [o["move"] for o in recs[1:]] == [2, 0], "the flip and the unbounded problem"
            t += 1
    assert seen["moves"] == {0, 1, 2} and all(seen[k] > 0 for k in ("tie", "upper", "lower", "outside", "er0", "nowinner_flip")), seen


# ---- 2. the width classes of slip_bstep_kernel ----

def width_case(rng, S, flip_winner=False):
    """two problems of n = 2 whose five scalars are of exactly S digits with one spare bit (32 S - 1 or 32 S - 2 bits: the bound
    max(bits) + 1 of the classification has S digits too): [0] a pivot with a finite range -- the comparison er |a'|, P = den
    a' and E = ev a' + N; [1] a flip with nothing eligible -- Dn = den d and E = (ev + sense er) d.  den, er and ev have
    exactly 32 bits (one digit), a'_r and d of [1] 32 (S - 1) - 1 bits: S digits by the factors' digit counts as well."""
    den, big = with_bits(rng, 32), 32 * (S - 1) - 1
    a_r, d1 = with_bits(rng, big), -with_bits(rng, big)
    bnd = dict(kind=[1, 0], lo=[-3, 0], hi=[0, 0], den=den)
    p0 = ([7, 5], [a_r, 0], 5)                                     # N = 7 den + 15, a' = a_r: a pivot, the range blocks later
    p1 = ([9, 4], [0, a_r], d1)                                    # entry 1 has no bound: nothing eligible
    ent = [(1, with_bits(rng, 32), with_bits(rng, 32)), (1, with_bits(rng, 32), -with_bits(rng, 32))]
    return [p0, p1], bnd, ent


def check_width_classes(lib_path, sizes=(4, 64, 128, 192, 256), memory=300):
    rng = random.Random(12)
    for S in sorted(set(sizes) | {s + 1 for s in sizes}):
        probs, bnd, ent = width_case(rng, S)
        den = bnd["den"]
        assert digits(den * probs[0][1][0]) == S and digits(den * probs[1][2]) == S
        assert digits(ent[0][1] * probs[0][1][0]) == S and digits(ent[0][2] * probs[0][1][0] + 7 * den + 15) == S
        _, paths, recs = run(lib_path, probs, bnd, ent, sense=1)
        assert [o["move"] for o in recs] == [1, 2]
        want = 1 if S <= 4 else 2 if S <= 256 else 3
        assert paths[16 + want] == 5 and sum(paths[16:20]) == 5, (S, paths)
    # the memory path: a'_r of `memory` digits
    a_r = with_bits(rng, 32 * memory)
    bnd = dict(kind=[1, 0], lo=[-3, 0], hi=[0, 0], den=6)
    _, paths, recs = run(lib_path, [([7, 5], [a_r, 0], 5), ([1, 1], [0, -a_r], -7)], bnd, [(1, 3, 2), (0, 0, 0)], sense=1)
    assert [o["move"] for o in recs] == [1, 0] and paths[19] == 3, paths


# ---- 3. the reduction: unit bounds and no entering data are Factorization.step ----

def rhs_of(probs):
    return slab([v for x, a, _ in probs for side in (x, a) for v in side])


def check_reduction(lib_path, name, transposes=(False, True), **kw):
    import slip_lu_amd as sl
    f, n, cols, q = case_handle(lib_path, name, **kw)
    try:
        f.run(0)
        unit = sl.Bounds(n, np.ones(n, np.int32), slab([0] * n))
        key = np.array([(7 * i) % 5 for i in range(n)], np.int32)
        for transpose in transposes:
            probs = handle_problems(n, cols, q, 31, transpose)
            b = rhs_of(probs)
            for sense, k in ((1, None), (-1, key)) if not transpose else ((1, key),):
                st = f.step(*b, nprob=len(probs), transpose=transpose, sense=sense, key=k)
                got = f.step_bounded(*b, unit, nprob=len(probs), transpose=transpose, sense=sense, key=k)
                paths = f.step_bounded_paths()
                rt = f.ratio_test_bounded(*b, unit, nprob=len(probs), transpose=transpose, sense=sense, key=k)
                assert all(np.array_equal(u, v) for u, v in zip((got.best, got.nties, got.neligible, *got.x, *got.d),
                                                                (st.best, st.nties, st.neligible, *st.x, *st.d)))
                assert all(np.array_equal(u, v) for u, v in zip((got.best, got.nties, got.neligible, got.side), rt))
                assert [int(m) for m in got.move] == [int(v >= 0) for v in st.best] and not got.ninexact.any()
                # E = xnum_best
                xe = oracle_lib.bigints(*st.x)
                same_slab(got.e, [xe[c * n + int(r)] if r >= 0 else 0 for c, r in enumerate(st.best)], "E = xnum_best")
                assert 1 in got.move and (sense != 1 or 0 in got.move)
                assert paths[13:16] == [int((got.move == m).sum()) for m in (0, 1, 2)] and sum(paths[8:12]) == n * len(probs)
                assert all(v >= 0 for v in f.step_bounded_ms())
    finally:
        f.close()


# ---- 4. the end-to-end proof ----

def boxed(n, xs, det, den, width):
    """bounds around the true values xs / det: floor(den x_i) -+ width over den, every entry boxed"""
    base = [(den * v) // det for v in xs]
    return dict(kind=[3] * n, lo=[v - width - i % 3 for i, v in enumerate(base)], hi=[v + 1 + width + i % 2 for i, v in enumerate(base)], den=den)


def check_proof(lib_path, name, negative_det=False, **kw):
    """a pivot proved against the replaced basis, a flip against the unchanged one: the solve of the right-hand side with the
    leaving variable moved to its bound and the entering variable's old value taken out equals R / Dn entry by entry (by
    cross-multiplication), E / Dn at the replaced position"""
    f, n, cols, q = case_handle(lib_path, name, **kw)
    try:
        f.run(0)
        det = oracle_lib.bigints(*f.pivots())[-1]
        if negative_det:
            assert det < 0, "det must be negative on this handle"
        x_rhs, a_rhs, _ = handle_problems(n, cols, q, 32, False)[0]
        b = slab(list(x_rhs) + list(a_rhs))
        xs = oracle_lib.bigints(*f.solve(*slab(x_rhs)))
        den, ev = 6, 5
        bnd = boxed(n, xs, det, den, 4)
        bounds = make_bounds(n, bnd)
        import slip_lu_amd as sl
        # the flip first (the handle stays as it is): a range of 1 / den is shorter than every step of this box
        flip = f.step_bounded(*b, bounds, sl.Entering(1, [1], 1, ev))
        assert int(flip.move[0]) == 2 and not flip.ninexact.any()
        R, Dn, E = oracle_lib.bigints(*flip.x), oracle_lib.bigints(*flip.d)[0], oracle_lib.bigints(*flip.e)[0]
        X = oracle_lib.bigints(*f.solve(*slab([den * u - 1 * v for u, v in zip(x_rhs, a_rhs)])))     # den b - sense er a_q
        assert Dn == den * det and all(u * Dn == r * det * den for u, r in zip(X, R)) and any(R)
        assert Fraction(E, Dn) == Fraction(ev + 1, den)
        # the pivot: the range does not block
        res = f.step_bounded(*b, bounds, sl.Entering(1, [1], 10 ** 6, ev))
        assert int(res.move[0]) == 1 and not res.ninexact.any()
        r, side = int(res.best[0]), int(res.side[0])
        R, Dn, E = oracle_lib.bigints(*res.x), oracle_lib.bigints(*res.d)[0], oracle_lib.bigints(*res.e)[0]
        beta = bnd["lo" if side < 0 else "hi"][r]                  # the leaving variable's bound, over den
        rhs = [den * u + ev * v for u, v in zip(x_rhs, a_rhs)]     # den b: the entering variable's old value taken out
        for i, v in cols[q[r]].items():
            rhs[i] -= beta * v                                     # the leaving variable at its bound
        new = {i: v for i, v in enumerate(a_rhs) if v}
        f.replace_column(q[r], list(new), list(new.values()))
        f.run(0)
        det2 = oracle_lib.bigints(*f.pivots())[-1]
        X = oracle_lib.bigints(*f.solve(*slab(rhs)))
        assert all(u * Dn == v * det2 * den for u, v in zip(X, R)), "X'' Dn == R det'' den"
        assert R[r] == E and any(X)
    finally:
        f.close()


# ---- 5. inexact divisions (caller slabs whose x, a, d do not belong together) ----

def check_inexact(lib_path):
    rng = random.Random(13)
    unit = lambda n: dict(kind=[1] * n, lo=[0] * n, hi=[0] * n, den=1)
    odd, m = with_bits(rng, 40) | 1, with_bits(rng, 90) | 1
    # entry 0 wins with x = 0 over alpha = 1 (nothing else is eligible): R_i = x_i / d for i > 0
    for d, xs, bad in ((8 * odd, [0, 4 * odd * m, 8 * odd * m, -4 * odd * m], 2),               # the trailing zero bits fail
                       (8 * odd, [0, 8 * (odd * m + 1), 8 * odd * m, 8 * (odd * m - 1)], 2),    # the odd part fails
                       (odd, [0, odd * m + 1, odd * m, -(odd * m) - 2], 2),                     # an odd D
                       (-odd, [0, odd * m, odd * m * 3, odd], 0)):
        a = [1 if d > 0 else -1, 0, 0, 0]                          # (sense * sign(d) * a_0 > 0)
        ok = ([0, 5 * d, -2 * d, d], a, d)
        res, paths, recs = run(lib_path, [(xs, a, d), ok], unit(4))
        assert [int(v) for v in res.ninexact] == [bad, 0] and paths[12] == bad and [o["move"] for o in recs] == [1, 1]
        lens = np.asarray(res.x[0][:4])
        assert int((lens == 0).sum()) == bad + 1                  # (the inexact entries and E = 0 come back empty)


# ---- 6. more than one staging group ----

def check_groups(lib_path, n=65):
    rng = random.Random(14)
    probs, bnd, ent = moves_case(rng, n, -(2 ** 40) - 15, 6, 1, 0)
    probs, ent = probs + probs[:2], ent + ent[:2]
    one, paths1, recs = run(lib_path, probs, bnd, ent)
    assert {o["move"] for o in recs} == {0, 1, 2}
    with one_problem_per_group():
        many, paths, _ = run(lib_path, probs, bnd, ent)
    assert same_result(one, many) and paths == paths1


# ---- 7. lifecycle and refusals ----

def check_lifecycle(lib_path, name="test_mat", **kw):
    import slip_lu_amd as sl
    f, n, cols, q = case_handle(lib_path, name, **kw)
    try:
        f.run(0)
        probs = handle_problems(n, cols, q, 41, False)[:1]
        b, rhs = rhs_of(probs), slab(probs[0][0])
        bnd = sl.Bounds(n, np.full(n, 3, np.int32), slab([-5] * n), slab([5] * n))
        ent = sl.Entering(1, [1], 10 ** 9, 3)
        services = lambda: f.solve(*rhs) + f.ratio_test_bounded(*b, bnd, winners=True) + tuple(
            v for s in [f.step(*b)] for v in (s.best, s.nties, s.neligible, s.ninexact, *s.x, *s.d))
        before = services()
        first = f.step_bounded(*b, bnd, ent)
        after = services()
        assert len(before) == len(after) and all(np.array_equal(u, v) for u, v in zip(before, after))
        again = f.step_bounded(*b, bnd, ent)
        f.rewind(n // 2)
        f.run(0)
        assert same_result(first, again) and same_result(first, f.step_bounded(*b, bnd, ent))
        assert int(first.move[0]) in (1, 2)
    finally:
        f.close()


def check_rejections(lib_path, name="test_mat", **kw):
    """SLIP_HIP_INCORRECT_INPUT (-3), nothing written"""
    import slip_lu_amd as sl
    from slip_lu_amd import _lib
    lib = _lib.load(lib_path)
    keep = [slab([5, -(2 ** 64), 1]), slab([1, 2 ** 64 + 1, -3]), slab([7]), slab([0]), slab([4]), slab([-4]), slab([2 ** 64])]
    X_, A_, D_, Z_, ER_, NEG_, EV_ = ((l.ctypes.data, x.ctypes.data if x.size else keep[0][1].ctypes.data, x.size) for l, x in keep)
    bnd = sl.Bounds(3, np.array([1, 3, 2], np.int32), slab([0, -1, 0]), slab([0, 9, 2 ** 64]), 3)
    badkind = sl.Bounds(3, np.array([1, 4, 2], np.int32), slab([0, -1, 0]), slab([0, 9, 4]))
    nolo = sl.Bounds(3, np.array([1, 3, 2], np.int32), None, slab([0, 9, 4]))
    fin, two = np.array([1], np.int32), np.array([2], np.int32)

    def entering(finite=fin, er=ER_, ev=EV_):
        e = _lib.EnteringRec()
        e.finite = None if finite is None else finite.ctypes.data
        if er is not None:
            e.erlen, e.erlimbs, e.er_limbs = er
        if ev is not None:
            e.evlen, e.evlimbs, e.ev_limbs = ev
        return e
    ents = dict(good=entering(), two=entering(finite=two), noer=entering(er=None), neg=entering(er=NEG_),
                ershort=entering(er=(ER_[0], ER_[1], 0)), evshort=entering(ev=(EV_[0], EV_[1], 0)),
                evhalf=entering(ev=(EV_[0], None, 1)), erhalf=entering(er=(None, ER_[1], 1)))
    res = [np.full(2, 77, np.int32) for _ in range(6)]
    R = [r.ctypes.data for r in res]
    outs = [C.c_void_p() for _ in range(6)] + [C.c_int64(55) for _ in range(3)]
    O = [C.byref(outs[0]), C.byref(outs[1]), C.byref(outs[6]), C.byref(outs[2]), C.byref(outs[3]), C.byref(outs[7]),
         C.byref(outs[4]), C.byref(outs[5]), C.byref(outs[8])]
    fn = lib.slip_hip_step_bounded
    good = (3, 1, *X_, *A_, *D_, bnd.ref(3), C.byref(ents["good"]), 1, None, *R, *O, None)

    def edit(base, **at):
        a = list(base)
        for k, v in at.items():
            a[int(k[1:])] = v
        return tuple(a)
    bad = [edit(good, _0=0), edit(good, _1=0), edit(good, _13=0), edit(good, _13=2),                  # n, nprob, sense
           edit(good, _2=None), edit(good, _3=None), edit(good, _5=None), edit(good, _6=None), edit(good, _8=None), edit(good, _9=None),
           edit(good, _4=X_[2] - 1), edit(good, _7=A_[2] - 1), edit(good, _10=0),                     # capacities
           edit(good, _8=Z_[0], _9=Z_[1], _10=Z_[2]),                                                # a zero d_c
           edit(good, _11=None), edit(good, _11=badkind.ref(3)), edit(good, _11=nolo.ref(3))]         # the bounds
    bad += [edit(good, _12=C.byref(ents[k])) for k in ("two", "noer", "neg", "ershort", "evshort", "evhalf", "erhalf")]
    bad += [edit(good, **{f"_{k}": None}) for k in range(15, 30)]                                     # any NULL output
    for args in bad:
        assert fn(*args) == -3, args[:2]
    assert all((r == 77).all() for r in res) and all(p.value is None for p in outs[:6]) and all(v.value == 55 for v in outs[6:])
    assert lib.slip_hip_step_bounded_paths(None) == -3 and lib.slip_hip_step_bounded_ms(None) == -3
    assert fn(*good) == 0 and res[4][0] in (1, 2)
    for p in outs[:6]:
        lib.slip_hip_free(p)
    assert fn(*edit(good, _12=None)) == 0                                                             # no entering data at all
    for p in outs[:6]:
        lib.slip_hip_free(p)
    with pytest.raises(ValueError):
        sl.step_bounded(2, *keep[0], *keep[1], *keep[2], bnd, lib_path=lib_path)
    with pytest.raises(ValueError):
        sl.Entering(2, [1])
    # on a handle
    f, n, cols, q = case_handle(lib_path, name, **kw)
    try:
        b = slab([(-1) ** t * (t % 7) for t in range(2 * n)])
        bl, bv = b[0].ctypes.data, b[1].ctypes.data
        hb = sl.Bounds(n, np.full(n, 3, np.int32), slab([-5] * n), slab([5] * n))
        ent = sl.Entering(1, [1], 2, 1)
        f.run(n // 2)
        assert f.info()["K"] < n
        with pytest.raises(sl.SlipError) as e:                     # an incomplete factorisation
            f.step_bounded(*b, hb, ent)
        assert e.value.code == -3
        f.run(0)
        res = [np.full(2, 77, np.int32) for _ in range(6)]
        R = [r.ctypes.data for r in res]
        step = lib.slip_hip_factor_step_bounded
        good = (f.h, 0, 1, bl, bv, hb.ref(n), ent.ref(1), 1, None, *R, *O, None)
        bad = [edit(good, _0=None), edit(good, _2=0), edit(good, _3=None), edit(good, _4=None), edit(good, _5=None), edit(good, _7=0), edit(good, _7=2)]
        bad += [edit(good, _6=C.byref(ents[k])) for k in ("two", "noer", "neg", "ershort", "evshort", "evhalf", "erhalf")]
        bad += [edit(good, **{f"_{k}": None}) for k in range(9, 24)]
        for p in outs[:6]:
            p.value = None
        for v in outs[6:]:
            v.value = 55
        for args in bad:
            assert step(*args) == -3, args[1:3]
        assert all((r == 77).all() for r in res) and all(p.value is None for p in outs[:6]) and all(v.value == 55 for v in outs[6:])
        assert lib.slip_hip_factor_step_bounded_paths(f.h, None) == -3 and lib.slip_hip_factor_step_bounded_paths(None, R[0]) == -3
        assert lib.slip_hip_factor_step_bounded_ms(f.h, None) == -3 and lib.slip_hip_factor_step_bounded_ms(None, R[0]) == -3
        with pytest.raises(ValueError):
            f.step_bounded(*b, hb, ent, nprob=2)
        with pytest.raises(ValueError):
            f.step_bounded(*b, hb, sl.Entering(2, [1, 0], [2, 2]))
        fac = f.download()
        tr = f.step_bounded(*b, hb, ent, transpose=True)
    finally:
        f.close()
    g = sl.Factorization.from_factors(fac, lib_path=lib_path, **{k: v for k, v in kw.items() if k in ("waves", "workers")})
    try:
        with pytest.raises(sl.SlipError) as e:                     # a handle around given factors holds no q
            g.step_bounded(*b, hb, ent)
        assert e.value.code == -3
        assert same_result(g.step_bounded(*b, hb, ent, transpose=True), tr)
    finally:
        g.close()
