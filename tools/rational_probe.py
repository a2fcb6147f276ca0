#!/usr/bin/env python3
"""Solve to reduced fractions (slip_hip_factor_solve_rational) against what a caller of `solve` does today: one
mpq_canonicalize per entry on one core.  Per case (complete-run goldens, one right-hand side) and for the widest class of
tests/golden/rational_corpus.json.gz (its denominators above 256 digits, through slip_hip_solution_to_rational), one JSON line:
  solve_ms / to_rational_ms   device ms of the substitution and of slip_reduce_kernel in the same solve_rational call
  paths                       entries settled by the lane pass, the register wave pass with g = 1 and g > 1, the memory class
  rational_wall_ms            host wall time of the whole call (for the corpus: upload, kernel, pack and download)
  gmp_ms                      system GMP's mpq_canonicalize on the same (xnum, det) pairs, one core, called through ctypes on
                              mpq_t set up beforehand; ctypes_call_us is the cost of one such call on 0/1, included per entry
  reduced                     entries whose denominator came out smaller than det
Each timed call is the second of its kind.  The fractions of both routes are compared.
usage: rational_probe.py case[,case...]"""
import ctypes as C
import ctypes.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import oracle_lib  # noqa: E402
import slip_lu_amd as sl  # noqa: E402
from conftest import load_case  # noqa: E402
from rational_helpers import fractions_of, load_corpus, padded_slab  # noqa: E402


class Mpz(C.Structure):
    _fields_ = [("alloc", C.c_int), ("size", C.c_int), ("d", C.c_void_p)]


class Mpq(C.Structure):
    _fields_ = [("num", Mpz), ("den", Mpz)]


GMP = C.CDLL(ctypes.util.find_library("gmp") or "libgmp.so.10")
GMP.__gmpq_canonicalize.argtypes = [C.POINTER(Mpq)]
GMP.__gmpz_set_str.argtypes = [C.POINTER(Mpz), C.c_char_p, C.c_int]
GMP.__gmpz_get_str.argtypes = [C.c_char_p, C.c_int, C.POINTER(Mpz)]
GMP.__gmpz_get_str.restype = C.c_char_p
GMP.__gmpz_sizeinbase.argtypes = [C.POINTER(Mpz), C.c_int]
GMP.__gmpz_sizeinbase.restype = C.c_size_t
GMP.__gmpq_init.argtypes = [C.POINTER(Mpq)]
GMP.__gmpq_clear.argtypes = [C.POINTER(Mpq)]


def wall(fn):
    t = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t) * 1e3


def mpz_int(z):
    buf = C.create_string_buffer(GMP.__gmpz_sizeinbase(C.byref(z), 16) + 2)
    return int(GMP.__gmpz_get_str(buf, 16, C.byref(z)).decode(), 16)


def gmp_canonicalize(pairs):
    """([(num, den)] as GMP canonicalises them, ms of the mpq_canonicalize calls alone, us of one call on 0/1)"""
    qs = (Mpq * len(pairs))()
    for q, (N, D) in zip(qs, pairs):
        GMP.__gmpq_init(C.byref(q))
        GMP.__gmpz_set_str(C.byref(q.num), format(N, "x").encode(), 16)
        GMP.__gmpz_set_str(C.byref(q.den), format(D, "x").encode(), 16)
    refs = [C.byref(q) for q in qs]
    canon = GMP.__gmpq_canonicalize
    t = time.perf_counter()
    for r in refs:
        canon(r)
    ms = (time.perf_counter() - t) * 1e3
    zero = Mpq()
    GMP.__gmpq_init(C.byref(zero))
    zr = C.byref(zero)
    t = time.perf_counter()
    for _ in range(1000):
        canon(zr)
    call_us = (time.perf_counter() - t) * 1e3
    out = [(mpz_int(q.num), mpz_int(q.den)) for q in qs]
    for q in qs:
        GMP.__gmpq_clear(C.byref(q))
    GMP.__gmpq_clear(C.byref(zero))
    return out, ms, call_us


def placed(vals, q):
    out = [None] * len(vals)
    for p, v in enumerate(vals):
        out[int(q[p])] = v
    return out


for name in [c for c in (sys.argv[1] if len(sys.argv) > 1 else "").split(",") if c]:
    e, fx = load_case(name)
    n, q = e["n"], np.asarray(fx["q"])
    g = sl.Factorization(n, fx["Ap"], fx["Ai"], fx["Alen"], fx["Alimbs"], q, pivot=e["pivot"], tol=e["tol"])
    g.run(0)
    det = oracle_lib.bigints(*g.pivots())[-1]
    b = (np.arange(n, dtype=np.int64) * 2654435761 % (1 << 32)) % 2001 - 1000
    bl, bx = sl.ints_to_slab(b)
    g.solve_rational(bl, bx)
    res, rwall = wall(lambda: g.solve_rational(bl, bx))
    solve_ms, red_ms, paths = g.solve_ms(), g.to_rational_ms(), g.to_rational_paths()
    x = oracle_lib.bigints(*g.solve(bl, bx))
    g.close()
    want, gmp_ms, call_us = gmp_canonicalize([(v, det) for v in x])
    got = fractions_of(res, n)
    print(json.dumps(dict(case=name, n=n, det_limbs=(det.bit_length() + 63) // 64, solve_ms=round(solve_ms, 3),
                          to_rational_ms=round(red_ms, 3), paths=paths, rational_wall_ms=round(rwall, 2), gmp_ms=round(gmp_ms, 3),
                          ctypes_call_us=round(call_us, 3), reduced=sum(1 for _, d in want if d != abs(det)),
                          identical=got == placed(want, q))), flush=True)

den, dpad, num, pad, _ = load_corpus()
keep = [c for c, D in enumerate(den) if abs(D).bit_length() > 256 * 32]
xlen, xlimbs = padded_slab([N for c in keep for N in num[c]], [p for c in keep for p in pad[c]])
dlen, dlimbs = padded_slab([den[c] for c in keep], [dpad[c] for c in keep])
n = len(num[0])
sl.solution_to_rational(n, xlen, xlimbs, dlen, dlimbs, nrhs=len(keep))
res, rwall = wall(lambda: sl.solution_to_rational(n, xlen, xlimbs, dlen, dlimbs, nrhs=len(keep)))
want, gmp_ms, call_us = gmp_canonicalize([(N, den[c]) for c in keep for N in num[c]])
print(json.dumps(dict(case="corpus, denominators above 256 digits", n=n * len(keep), paths=sl.solution_to_rational_paths(),
                      rational_wall_ms=round(rwall, 2), gmp_ms=round(gmp_ms, 3), ctypes_call_us=round(call_us, 3),
                      identical=fractions_of(res, n * len(keep)) == want)), flush=True)
