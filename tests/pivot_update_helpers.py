"""Shared by tests/test_emu_pivot_update.py (the emulator build) and tests/test_gpu_pivot_update.py (the product on the device):
the exact pivot update R_i = (P V_i - T A_i) / D (slip_hip_pivot_update on caller slabs; slip_hip_factor_solve_update and
slip_hip_factor_step fused with a solve on a handle).  The oracle is Python integers and fractions: every result is compared
with the exact quotient, every comparison is exact equality of normalised slabs, and a step is also proved end to end against
a fresh factorisation of the replaced basis by cross-multiplication.  lib_path None is the product library."""
import contextlib
import ctypes as C
import os
import random
from fractions import Fraction

import numpy as np
import pytest

import oracle_lib
from check_helpers import columns, slab
from conftest import load_case
from product_helpers import same_slab
from ratio_helpers import oracle_ties, padded_slab, pick

SIZES = (2, 4, 5, 64, 65, 128, 129, 192, 193, 256, 257, 300)          # digits of the wider product


def digits(v):
    return (abs(v).bit_length() + 31) // 32


# ---- the oracle ----

def classify(P, V, T, A, D):
    """the path of one entry, as the header defines it: 0 both terms zero, 1 a lane (both products of at most four digits by
    the factors' digit counts, D of at most two), 2 registers (the bound max(bits) + 1 of the numerator fits 256 digits), 3
    memory"""
    s1, s2 = bool(P and V), bool(T and A)
    if not s1 and not s2:
        return 0
    b1 = abs(P).bit_length() + abs(V).bit_length() if s1 else 0
    b2 = abs(T).bit_length() + abs(A).bit_length() if s2 else 0
    w1, w2 = (digits(P) + digits(V) if s1 else 0), (digits(T) + digits(A) if s2 else 0)
    if w1 <= 4 and w2 <= 4 and (D is None or digits(D) <= 2):
        return 1
    return 2 if (max(b1, b2) + 1 + 31) // 32 <= 256 else 3


def quotient(P, V, T, A, D):
    """(the exact quotient or 0, inexact)"""
    N = P * V - T * A
    if D is None:
        return N, 0
    if N % D:
        return 0, 1
    q = abs(N) // abs(D)
    return (q if (N < 0) == (D < 0) else -q), 0


def run(lib_path, probs, place=None, pad=False):
    """one call of slip_hip_pivot_update on [(P, T, D or None, Vs, As), ...] (every problem with a D or none of them) against
    the oracle; returns the path counts.  pad: high zero limbs on every operand."""
    import slip_lu_amd as sl
    n, nprob = len(probs[0][3]), len(probs)
    pe = [t % 3 for t in range(n * nprob)] if pad else None
    ps = [1 + c % 2 for c in range(nprob)] if pad else None
    v = padded_slab([x for p in probs for x in p[3]], pe)
    a = padded_slab([x for p in probs for x in p[4]], pe)
    P, T = padded_slab([p[0] for p in probs], ps), padded_slab([p[1] for p in probs], ps)
    d = None if probs[0][2] is None else padded_slab([p[2] for p in probs], ps)
    rlen, rlimbs, nin = sl.pivot_update(n, *v, *a, P, T, d=d, place=place, nprob=nprob, lib_path=lib_path)
    want, bad, paths = [], [], [0, 0, 0, 0]
    for c, (p, t, dd, vs, avs) in enumerate(probs):
        bad.append(0)
        for i, (x, y) in enumerate(zip(vs, avs)):
            if place is not None and place[c] == i:
                want.append(t); paths[0] += 1
                continue
            q, inexact = quotient(p, x, t, y, dd)
            want.append(q); bad[-1] += inexact
            paths[classify(p, x, t, y, dd)] += 1
    same_slab((rlen, rlimbs), want, "the quotients")
    assert [int(k) for k in nin] == bad, "ninexact"
    got = sl.pivot_update_paths(lib_path=lib_path)
    assert got[:4] == paths and got[4] == sum(bad) and got[5:] == [0, 0, 0], (got, paths)
    return got


@contextlib.contextmanager
def one_problem_per_group():
    """the smallest staging budget: every problem of a call is staged, formed and packed on its own"""
    os.environ["SLIP_HIP_PRODUCT_STAGE_KB"] = "1"
    try:
        yield
    finally:
        del os.environ["SLIP_HIP_PRODUCT_STAGE_KB"]


def with_bits(rng, bits):
    """a random integer of exactly `bits` bits whose two leading bits are set"""
    return (3 << (bits - 2)) | rng.getrandbits(bits - 2) if bits >= 2 else 1


def mid_bits(rng, bits):
    """a random integer in [5/8, 3/4) * 2^bits: it keeps its `bits` bits when less than 2^(bits - 3) is added or taken away"""
    return (5 << (bits - 3)) | rng.getrandbits(bits - 3)


def divisible_problem(rng, n, pbits, vbits, D, sp=1, st=1):
    """(P, T, D, Vs, As) with V_i = D v_i + T k_i and A_i = D a_i + P k_i, so that P V_i - T A_i = D (P v_i - T a_i): P and T of
    pbits bits, every V_i and A_i of exactly vbits bits (D at least three bits below)"""
    assert abs(D).bit_length() <= vbits - 3
    P, T = sp * with_bits(rng, pbits), st * with_bits(rng, pbits)
    kb = max(1, min(40, vbits - pbits - 3))
    Vs, As = [], []
    for _ in range(n):
        k = rng.getrandbits(kb) if vbits - pbits - 3 >= 1 else 0
        sv, sa = rng.choice((1, -1)), rng.choice((1, -1))
        tv, ta = sv * mid_bits(rng, vbits), sa * mid_bits(rng, vbits)
        V, A = D * ((tv - T * k) // D) + T * k, D * ((ta - P * k) // D) + P * k
        assert abs(V).bit_length() == vbits and abs(A).bit_length() == vbits
        Vs.append(V); As.append(A)
    return P, T, D, Vs, As


# ---- 1. width classes ----

def width_cases(S):
    """the (pbits, vbits, D) of size S: the products have exactly S digits and 32 S - 1 or 32 S - 2 bits, so that the bound of
    the numerator (one more bit) has S digits too.  D = odd << tz, the odd part of 12 bits (one digit) or about half the
    product's length, tz in (0, 1, 33, 64), every second D negative; a D that would not leave V three bits is not possible at
    this size (a numerator of two digits has no divisor with 64 trailing zeros) and is left out."""
    pbits = 24 if S == 2 else 32 * max(1, S // 8)
    vbits = 32 * S - 1 - pbits
    out = []
    for half in (0, 1):
        for tz in (0, 1, 33, 64):
            ob = min(16 * S, vbits - 3 - tz) if half else 12
            if ob < 2 or ob + tz > vbits - 3:
                continue
            out.append((pbits, vbits, ob, tz))
    return out


def check_width_classes(lib_path, sizes=SIZES):
    rng = random.Random(5)
    seen = [0, 0, 0, 0]
    for S in sizes:
        cases = width_cases(S)
        assert len(cases) >= 2
        if len(cases) % 2:
            cases.append(cases[0])
        for t in range(0, len(cases), 2):
            probs = []
            for u, (pbits, vbits, ob, tz) in enumerate(cases[t:t + 2]):
                D = (-1 if u else 1) * ((with_bits(rng, ob) | 1) << tz)
                p = divisible_problem(rng, 3, pbits, vbits, D, rng.choice((1, -1)), rng.choice((1, -1)))
                assert max(digits(p[0] * x) for x in p[3]) == S and max(digits(p[1] * y) for y in p[4]) == S
                probs.append(p)
            got = run(lib_path, probs)
            want = 1 if S <= 4 and all(digits(p[2]) <= 2 for p in probs) else (2 if S <= 256 else 3)
            if all(digits(p[2]) <= 2 for p in probs) or S > 4:
                assert got[want] == 6, (S, got)
            for k in range(4):
                seen[k] += got[k]
    assert seen[1] > 0 and seen[2] > 0 and seen[3] > 0, seen


# ---- 2. signs, zeros, no division ----

def check_signs_and_zeros(lib_path):
    rng = random.Random(6)
    P0, T0 = 2 ** 70 + 9, 3 ** 40 + 2                             # coprime
    assert Fraction(P0, T0).denominator == T0
    for wide in (0, 1):
        D0 = (2 ** 100 + 7) * 8 if wide else 24
        unit = 2 ** 180 if wide else 1                             # (wide: registers; else the numerators of the lane fit four digits)
        p0, t0 = (P0, T0) if wide else (2 ** 20 + 7, 3 ** 12 + 2)
        v1 = pow(p0, -1, t0); a1 = (p0 * v1 - 1) // t0             # p0 v1 - t0 a1 = 1
        for div in (True, False):
            for pad in (False, True):
                probs = []
                for sp, st, sd in ((1, 1, 1), (-1, 1, -1), (1, -1, -1), (-1, -1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, -1), (-1, -1, -1)):
                    P, T, D = sp * p0, st * t0, sd * D0
                    ents = []                                      # (v, a, k): V = D v + T k, A = D a + P k
                    for sv in (1, -1):
                        for sa in (1, -1):
                            ents.append((sv * (unit + rng.getrandbits(18)), sa * (unit + rng.getrandbits(18)), 0))
                            ents.append((sv * unit, sa * unit, rng.getrandbits(9) + 1))
                    ents += [(0, 5 * unit, 0), (7 * unit, 0, 0), (0, 0, 0)]          # V = 0, A = 0, both
                    ents += [(T * 11, P * 11, 3), (v1 * sp, a1 * st, 0), (-v1 * sp, -a1 * st, 0)]     # to 0, D and -D: quotients 0, 1, -1
                    Vs, As = [D * v + T * k for v, a, k in ents], [D * a + P * k for v, a, k in ents]
                    probs.append((P, T, D if div else None, Vs, As))
                    if div:
                        assert [quotient(P, x, T, y, D)[0] for x, y in zip(Vs[-3:], As[-3:])] == [0, 1, -1]
                    else:
                        assert [P * x - T * y for x, y in zip(Vs[-3:], As[-3:])] == [0, D, -D]
                for t in range(0, 8, 2):
                    got = run(lib_path, probs[t:t + 2], pad=pad)
                    assert got[0] == 2 and got[1 if not wide else 2] > 0, got
                if pad:                                            # T = 0 and P = 0 (every V and A a multiple of D)
                    mul = D0 if div else 1
                    z = [(0 if c == 0 else P, 0 if c == 1 else T, D, [mul * x for x in Vs], [mul * y for y in As])
                         for c, (P, T, D, Vs, As) in enumerate(probs[:2])]
                    run(lib_path, z, pad=True)


def check_lane_carry(lib_path):
    """four-digit products whose signed sum reaches 2^128 (the lane's carry), divided by a unit, by 2 (the carry shifted back in),
    by odd and even D of two digits, and not divided: the quotient by +-1 has five digits"""
    m = 2 ** 64 - 1                                                # = 3 * 5 * 17 * 257 * 641 * 65537 * 6700417
    f = 641 * 6700417                                              # 2^32 + 1: two digits, odd
    assert digits(f) == 2 and m % f == 0 and digits(2 * m * m) == 5
    for D in (1, -1, 2, -2, 3, f, -f, 2 * f, None):
        probs = [(sp * m, -sp * m, D, [m, -m, m - 1], [m, -m, 1]) for sp in (1, -1)]
        if D is not None:
            assert all(classify(P, x, T, y, D) == 1 and quotient(P, x, T, y, D)[1] == 0 for P, T, _, Vs, As in probs for x, y in zip(Vs[:2], As[:2]))
            probs = [(P, T, D, [Vs[0], Vs[1], abs(D) * Vs[2]], [As[0], As[1], abs(D) * As[2]]) for P, T, _, Vs, As in probs]
        got = run(lib_path, probs)
        assert got[1] >= 4 and got[4] == 0, (D, got)


# ---- 3. inexact ----

def check_inexact(lib_path):
    rng = random.Random(7)
    for vbits, want in ((60, 1), (3000, 2), (9000, 3)):
        D = 24 * 5 if want == 1 else ((with_bits(rng, 40) | 1) << 3)
        ok = divisible_problem(rng, 3, 24, vbits, D)
        other = divisible_problem(rng, 3, 24, vbits, -D)
        assert ok[0] % D and all(classify(ok[0], x, ok[1], y, D) == want for x, y in zip(ok[3], ok[4]))
        base = run(lib_path, [ok, other])
        assert base[4] == 0 and base[want] == 6
        # one V_i plus one: the numerator moves by P, which D does not divide
        for i in (0, 2):
            Vs = list(ok[3]); Vs[i] += 1
            got = run(lib_path, [(ok[0], ok[1], D, Vs, ok[4]), other])
            assert got[4] == 1
            got = run(lib_path, [other, (ok[0], ok[1], D, Vs, ok[4])])
            assert got[4] == 1
            with one_problem_per_group():
                assert run(lib_path, [other, (ok[0], ok[1], D, Vs, ok[4]), other])[4] == 1
        # P = 1: the numerator is V - T A, chosen freely.  D = 8 * odd: only the trailing zero bits fail (4 odd m), only the
        # odd part fails (8 (odd m + 1)); D odd: the high-digit test alone
        T, As = ok[1], ok[4]
        odd = D >> 3 if want > 1 else 15
        m = with_bits(rng, vbits - 8) | 1
        for Dv, Ns in ((8 * odd, [4 * odd * m, 8 * odd * m, -4 * odd * m]), (8 * odd, [8 * (odd * m + 1), 8 * odd * m, 8 * (odd * m - 1)]),
                       (odd, [odd * m + 1, odd * m, -(odd * m) - 2]), (-odd, [odd * m + 1, odd * m, odd * (m << 70) + 1])):
            prob = (1, T, Dv, [N + T * y for N, y in zip(Ns, As)], As)
            assert [quotient(1, x, T, y, Dv)[1] for x, y in zip(prob[3], As)] == [1, 0, 1]
            got = run(lib_path, [prob, other])
            assert got[4] == 2


# ---- 4. placement and geometry ----

def check_geometry(lib_path, sizes):
    rng = random.Random(8)
    for n in sizes:
        probs = []
        for c in range(3):
            D = (rng.getrandbits(20) | 1) << c
            p = divisible_problem(rng, n, 24, 60, D, 1, -1 if c else 1)
            wide = divisible_problem(rng, n, 40, 2200, D)           # every seventh entry in registers
            Vs = [wide[3][i] if i % 7 == 3 else p[3][i] for i in range(n)]
            As = [wide[4][i] if i % 7 == 3 else p[4][i] for i in range(n)]
            Vs = [D * (x // D) for x in Vs]; As = [D * (y // D) for y in As]       # (one P and T for both kinds: k = 0)
            probs.append((p[0], p[1], D, Vs, As))
        place = np.array([-1, 0, n - 1], np.int32)
        got = run(lib_path, probs, place=place)
        assert got[0] >= 2 and got[1] > 0 and (n < 4 or got[2] > 0)
        run(lib_path, probs)
        if n == 65:
            with one_problem_per_group():
                assert run(lib_path, probs, place=place) == got


# ---- 5. on handles ----

def case_handle(lib_path, name, **kw):
    import slip_lu_amd as sl
    _, fix = load_case(name)
    n, Ap, Ai, Alen, Alimbs, q = len(fix["q"]), fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"]
    cols = columns(n, Ap, Ai, oracle_lib.bigints(Alen, Alimbs))
    return sl.Factorization(n, Ap, Ai, Alen, Alimbs, q, lib_path=lib_path, **kw), n, cols, [int(j) for j in q]


def basis_times(n, cols, q, w, transpose):
    """A(:,q) w by row, or A(:,q)^T w by position"""
    out = [0] * n
    for k in range(n):
        for i, v in cols[q[k]].items():
            if transpose:
                out[k] += v * w[i]
            else:
                out[i] += v * w[k]
    return out


def handle_problems(n, cols, q, seed, transpose):
    """[(x side, a side, w)]: the a side is A(:,q) w (transposed: A(:,q)^T w), so that its solve is det * w and the eligible
    entries are those with sense * w_i > 0: a mixed w, an unbounded one (w <= 0 under sense 1) and one whose x side is three
    times its a side (every eligible entry ties)"""
    rng = random.Random(seed)
    mixed = lambda: [rng.choice((-3, -1, 0, 1, 2, 5)) for _ in range(n)]
    w0, w1, w2 = mixed(), [-abs(v) for v in mixed()], mixed()
    w0[n // 2], w2[0], w2[n - 1] = 2, 1, 4
    b0 = [rng.randrange(-9, 10) for _ in range(n)]
    b1 = [rng.randrange(-99, 100) for _ in range(n)]
    a0, a1, a2 = (basis_times(n, cols, q, w, transpose) for w in (w0, w1, w2))
    return [(b0, a0, w0), (b1, a1, w1), ([3 * v for v in a2], a2, w2)]


def step_against_python(f, lib_path, n, probs, transpose, sense, key, memory_path=False, cross=True):
    """one step against the handle's own solve and the formula; returns (the solve's sides, the expected winners, the result)"""
    nprob = len(probs)
    b = slab([v for x, a, _ in probs for side in (x, a) for v in side])
    det = oracle_lib.bigints(*f.pivots())[-1]
    num = oracle_lib.bigints(*(f.solve_transpose if transpose else f.solve)(*b, nrhs=2 * nprob))
    sides = [(num[2 * c * n:(2 * c + 1) * n], num[(2 * c + 1) * n:(2 * c + 2) * n]) for c in range(nprob)]
    for (_, _, w), (_, an) in zip(probs, sides):
        assert an == [det * v for v in w], "the a side is det * w by construction"
    want = [pick(*oracle_ties(x, a, sense, 1 if det > 0 else -1), key) for x, a in sides]
    for (_, _, w), wt in zip(probs, want):
        assert (wt[0] >= 0) == any(sense * v > 0 for v in w), "an eligible entry gives a winner"
    res = f.step(*b, nprob=nprob, transpose=transpose, sense=sense, key=key)
    paths, ms, rms, rpaths = f.update_paths(), f.update_ms(), f.ratio_test_ms(), f.ratio_test_paths()
    got = [(int(res.best[c]), int(res.nties[c]), int(res.neligible[c])) for c in range(nprob)]
    assert got == want, (transpose, sense)
    if cross:
        rt = f.ratio_test(*b, nprob=nprob, transpose=transpose, sense=sense, key=key)
        assert got == [(int(rt[0][c]), int(rt[1][c]), int(rt[2][c])) for c in range(nprob)], (transpose, sense)
    xs, ds = [], []
    for (x, a), (r, _, _) in zip(sides, want):
        if r < 0:
            xs += [0] * n; ds.append(0)
            continue
        for i in range(n):
            N = a[r] * x[i] - x[r] * a[i]
            assert N % det == 0
            xs.append(x[r] if i == r else N // det)
        ds.append(a[r])
    same_slab(res.x, xs, "the new numerators")
    same_slab(res.d, ds, "the new denominators")
    assert [int(v) for v in res.ninexact] == [0] * nprob
    assert sum(paths[:4]) == n * nprob and paths[4:] == [0, 0, 0, 0] and ms[0] >= 0 and ms[1] == rms
    assert rpaths[0] == sum(w[2] for w in want)
    if memory_path:                                        # (one substitution of this golden takes 0.6 s on the device)
        assert paths[3] > 0, "the memory path was not reached"
    if memory_path or not cross:
        return sides, want, res
    # the fused update against the handle-less one on the downloaded numerators
    import slip_lu_amd as sl
    ok = [c for c in range(nprob) if want[c][0] >= 0]
    P, T = [sides[c][1][want[c][0]] if c in ok else 1 for c in range(nprob)], [sides[c][0][want[c][0]] if c in ok else 2 for c in range(nprob)]
    place = np.array([want[c][0] for c in range(nprob)], np.int32)
    fused = f.solve_update(*b, slab(P), slab(T), nprob=nprob, transpose=transpose, place=place)
    plain = sl.pivot_update(n, *slab([v for x, _ in sides for v in x]), *slab([v for _, a in sides for v in a]), slab(P), slab(T),
                            d=slab([det] * nprob), place=place, nprob=nprob, lib_path=lib_path)
    assert all(np.array_equal(u, v) for u, v in zip(fused, plain))
    for c in ok:
        assert np.array_equal(fused[0][c * n:(c + 1) * n], res.x[0][c * n:(c + 1) * n])
    return sides, want, res


def end_to_end(f, lib_path, n, cols, q, probs, cross=True):
    """the proof of the step and of the dual form: replace the leaving column by the entering one, factorise, solve again"""
    x_rhs, a_rhs, _ = probs[0]
    sides, want, res = step_against_python(f, lib_path, n, probs[:1], False, 1, None, cross=cross)
    r = want[0][0]
    assert r >= 0
    det = oracle_lib.bigints(*f.pivots())[-1]
    x1, d1 = oracle_lib.bigints(*res.x), oracle_lib.bigints(*res.d)[0]
    A_r = sides[0][1][r]
    assert d1 == A_r
    # the duals: Y' = (A_r Y + D_q R) / det over A_r with Y, R the transposed solves of c_B and e_r, D_q = det c_q - a_q^T Y
    rng = random.Random(21)
    cB, cq = [rng.randrange(-9, 10) for _ in range(n)], 7
    e_r = [int(k == r) for k in range(n)]
    dual_rhs = slab(cB + e_r)
    Y = oracle_lib.bigints(*f.solve_transpose(*slab(cB)))
    D_q = det * cq - sum(a * y for a, y in zip(a_rhs, Y))
    y1 = f.solve_update(*dual_rhs, A_r, -D_q, transpose=True)
    assert [int(v) for v in y1[2]] == [0]
    y1 = oracle_lib.bigints(y1[0], y1[1])
    new = {i: v for i, v in enumerate(a_rhs) if v}
    f.replace_column(q[r], list(new), list(new.values()))
    f.run(0)
    det2 = oracle_lib.bigints(*f.pivots())[-1]
    x2 = oracle_lib.bigints(*f.solve(*slab(x_rhs)))
    assert abs(det2) == abs(d1)
    assert all(u * d1 == v * det2 for u, v in zip(x2, x1)), "X'' d == x det''"
    cB2 = list(cB); cB2[r] = cq
    y2 = oracle_lib.bigints(*f.solve_transpose(*slab(cB2)))
    assert all(u * A_r == v * det2 for u, v in zip(y2, y1)), "Y'' A_r == Y' det''"
    assert any(y2) and any(x2)


def check_golden(lib_path, name, memory_path=False, light=False, transposes=(False, True), proof=False, cross=True, negative_det=False, **kw):
    """steps on a complete golden against Python (light, for the emulator: two problems and one combination per orientation;
    memory_path, the widest golden: the same; cross=False leaves out the second and third substitution that compare the step
    with ratio_test and solve_update with pivot_update); proof: the end-to-end proof and the dual form; negative_det: this
    handle must have det < 0, where the eligible sign of anum is the opposite of sense (test_mat has: its steps and its proof
    then run through that branch)"""
    f, n, cols, q = case_handle(lib_path, name, **kw)
    try:
        f.run(0)
        if negative_det:
            assert oracle_lib.bigints(*f.pivots())[-1] < 0, "det must be negative on this handle"
        key = np.array([(7 * i) % 5 for i in range(n)], np.int32)
        for transpose in transposes:
            probs = handle_problems(n, cols, q, 31, transpose)
            if light or memory_path:
                probs = probs[:2]
            for sense, k in ((1, None), (-1, key)) if not (light or memory_path) else (((1, None),) if not transpose else ((-1, key),)):
                _, want, _ = step_against_python(f, lib_path, n, probs, transpose, sense, k, memory_path)
                if sense == 1:
                    assert want[1][0] == -1, "the unbounded problem"
        if proof:
            end_to_end(f, lib_path, n, cols, q, handle_problems(n, cols, q, 32, False), cross)
    finally:
        f.close()


# ---- 6. lifecycle ----

def check_lifecycle(lib_path, name="gen_n40", **kw):
    import slip_lu_amd as sl
    f, n, cols, q = case_handle(lib_path, name, **kw)
    try:
        f.run(0)
        probs = handle_problems(n, cols, q, 41, False)[:1]
        b = slab([v for x, a, _ in probs for side in (x, a) for v in side])
        rhs = slab(probs[0][0])
        M = sl.SparseMatrix(n, n, np.cumsum([0] + [len(c) for c in cols]).astype(np.int64), np.array([i for c in cols for i in c], np.int32),
                            *slab([v for c in cols for v in c.values()]), lib_path=lib_path)
        bnd = sl.Bounds(n, np.full(n, 3, np.int32), slab([-5] * n), slab([5] * n))
        def services():
            return (f.solve(*rhs) + f.ratio_test(*b, winners=True) + f.price(M, *rhs, winners=True)
                    + f.bound_test(*rhs, bnd, winners=True))
        try:
            before = services()
            first = f.step(*b)
            after = services()
            assert len(before) == len(after) and all(np.array_equal(u, v) for u, v in zip(before, after))
            again = f.step(*b)
            f.rewind(n // 2)
            f.run(0)
            third = f.step(*b)
            for other in (again, third):
                assert all(np.array_equal(u, v) for u, v in zip((first.best, first.nties, first.neligible, first.ninexact, *first.x, *first.d),
                                                                (other.best, other.nties, other.neligible, other.ninexact, *other.x, *other.d)))
            assert first.best[0] >= 0
        finally:
            M.close()
    finally:
        f.close()


# ---- 7. rejections: SLIP_HIP_INCORRECT_INPUT (-3), nothing written ----

def check_rejections(lib_path, name="test_mat", **kw):
    import slip_lu_amd as sl
    from slip_lu_amd import _lib
    lib = _lib.load(lib_path)
    keep = [slab([5, -(2 ** 64), 1]), slab([1, 2 ** 64 + 1, -3]), slab([7]), slab([-2 ** 70]), slab([3]), slab([0])]
    V_, A_, P_, T_, D_, Z_ = ((l.ctypes.data, x.ctypes.data if x.size else keep[0][1].ctypes.data, x.size) for l, x in keep)
    place, high, low, past = (np.array([v], np.int32) for v in (1, 3, -2, 10 ** 6))
    nin = np.full(2, 77, np.int32)
    pl, px, nl = C.c_void_p(), C.c_void_p(), C.c_int64(55)
    outs = (C.byref(pl), C.byref(px), C.byref(nl))
    NONE = (None, None, 0)
    short = lambda s: (s[0], s[1], s[2] - 1)
    fn = lib.slip_hip_pivot_update
    good = (3, 1, *V_, *A_, *P_, *T_, *D_, place.ctypes.data, nin.ctypes.data, *outs, None)
    def edit(**at):
        a = list(good)
        for k, v in at.items():
            a[int(k[1:])] = v
        return tuple(a)
    bad = [edit(_0=0), edit(_0=-1), edit(_1=0),                                                     # n <= 0, nprob < 1
           edit(_2=None), edit(_3=None), edit(_5=None), edit(_6=None), edit(_8=None), edit(_9=None), edit(_11=None), edit(_12=None),
           edit(_14=None), edit(_15=None),                                                           # exactly one of dlen / dlimbs
           (3, 1, *V_, *A_, *P_, *T_, *Z_, None, nin.ctypes.data, *outs, None),                     # a zero D_c
           edit(_4=V_[2] - 1), edit(_7=A_[2] - 1), edit(_10=P_[2] - 1), edit(_13=T_[2] - 1), edit(_16=D_[2] - 1),      # capacities
           edit(_17=high.ctypes.data), edit(_17=low.ctypes.data),              # place
           edit(_18=None), edit(_19=None), edit(_20=None), edit(_21=None)]                           # ninexact, a partial output triple
    for args in bad:
        assert fn(*args) == -3, args[:2]
    assert (nin == 77).all() and pl.value is None and px.value is None and nl.value == 55
    assert lib.slip_hip_pivot_update_paths(None) == -3
    assert fn(*good) == 0 and nin[0] == 1
    lib.slip_hip_free(pl); lib.slip_hip_free(px)
    assert fn(*edit(_14=None, _15=None, _16=0)) == 0 and nin[0] == 0                                 # no division
    lib.slip_hip_free(pl); lib.slip_hip_free(px)
    with pytest.raises(ValueError):
        sl.pivot_update(2, *keep[0], *keep[1], 7, 3, lib_path=lib_path)
    with pytest.raises(ValueError):
        sl.pivot_update(3, *keep[0], *keep[1], [7, 7], 3, lib_path=lib_path)
    # on a handle
    f, n, cols, q = case_handle(lib_path, name, **kw)
    try:
        b = slab([(-1) ** t * (t % 7) for t in range(2 * n)])
        bl, bv = b[0].ctypes.data, b[1].ctypes.data
        res = [np.full(2, 77, np.int32) for _ in range(4)]
        R = [r.ctypes.data for r in res]
        ql, qx, qn = C.c_void_p(), C.c_void_p(), C.c_int64(55)
        outs2 = (C.byref(ql), C.byref(qx), C.byref(qn))
        pl, px, nl = C.c_void_p(), C.c_void_p(), C.c_int64(55)
        outs = (C.byref(pl), C.byref(px), C.byref(nl))
        f.run(n // 2)
        assert f.info()["K"] < n
        for call in (lambda: f.step(*b), lambda: f.solve_update(*b, 3, 5)):       # an incomplete factorisation
            with pytest.raises(sl.SlipError) as e:
                call()
            assert e.value.code == -3
        f.run(0)
        step, upd = lib.slip_hip_factor_step, lib.slip_hip_factor_solve_update
        good = (f.h, 0, 1, bl, bv, 1, None, *R, *outs, *outs2, None)
        def edit(**at):
            a = list(good)
            for k, v in at.items():
                a[int(k[1:])] = v
            return tuple(a)
        bad = [edit(_0=None), edit(_2=0), edit(_3=None), edit(_4=None), edit(_5=0), edit(_5=2)] + [edit(**{f"_{k}": None}) for k in range(7, 17)]
        for args in bad:
            assert step(*args) == -3, args[1:3]
        good = (f.h, 0, 1, bl, bv, *P_, *T_, place.ctypes.data, R[3], *outs, None)
        bad = [edit(_0=None), edit(_2=0), edit(_3=None), edit(_4=None), edit(_5=None), edit(_6=None), edit(_8=None), edit(_9=None),
               edit(_7=P_[2] - 1), edit(_10=T_[2] - 1), edit(_11=past.ctypes.data), edit(_11=low.ctypes.data), edit(_12=None), edit(_13=None), edit(_14=None), edit(_15=None)]
        for args in bad:
            assert upd(*args) == -3, args[1:3]
        assert all((r == 77).all() for r in res) and all(p.value is None for p in (pl, px, ql, qx)) and nl.value == 55 and qn.value == 55
        assert lib.slip_hip_factor_update_paths(f.h, None) == -3 and lib.slip_hip_factor_update_paths(None, R[0]) == -3
        assert lib.slip_hip_factor_update_ms(f.h, None) == -3 and lib.slip_hip_factor_update_ms(None, R[0]) == -3
        with pytest.raises(ValueError):
            f.step(*b, nprob=2)
        with pytest.raises(ValueError):
            f.step(*b, key=np.zeros(n + 1, np.int32))
        with pytest.raises(ValueError):
            f.solve_update(*b, [3, 4], 5)
        fac = f.download()
        tr = f.step(*b, transpose=True)
    finally:
        f.close()
    g = sl.Factorization.from_factors(fac, lib_path=lib_path, **{k: v for k, v in kw.items() if k in ("waves", "workers")})
    try:
        for call in (lambda: g.step(*b), lambda: g.solve_update(*b, 3, 5)):       # a handle around given factors holds no q
            with pytest.raises(sl.SlipError) as e:
                call()
            assert e.value.code == -3
        got = g.step(*b, transpose=True)
        assert all(np.array_equal(u, v) for u, v in zip((got.best, *got.x, *got.d), (tr.best, *tr.x, *tr.d)))
    finally:
        g.close()
