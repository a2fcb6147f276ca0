#!/usr/bin/env python3
"""Solve straight to correctly rounded floats (slip_hip_factor_solve_mpfr) against the route it replaces: solve_rational, every
reduced fraction to the host, then mpfr_set_q per entry on one core.  Resident factors, one and sixteen right-hand sides,
precisions 53, 128 and 1000 under MPFR_RNDN.  Per case, nrhs and precision, one JSON line:
  solve_ms / to_mpfr_ms     device ms of the substitution and of slip_mpfr_kernel in the same solve_mpfr call
  to_rational_ms            device ms of slip_reduce_kernel in the solve_rational call on the same right-hand sides
  paths                     shares of the entries settled by the lane pass within 64 bits, the long division with a denominator
                            of at most 256 digits and with a wider one, and as zero
  mpfr_wall_ms              host wall time of solve_mpfr
  rational_wall_ms          host wall time of solve_rational for the same right-hand sides
  set_q_ms                  system MPFR's mpfr_set_q on the reduced fractions, one core, through ctypes on mpq_t and mpfr_t set up
                            beforehand: timed on the first right-hand side (the others repeat it), times nrhs -- for 16 an
                            extrapolation, not a measurement
  d2h_mpfr / d2h_rational   bytes handed back to the caller: 10 + 8 * ceil(prec / 64) per entry, against 8 per entry + the limbs
                            of both slabs
Each timed call is the second of its kind (the first loads the code and sizes the buffers).  The floats of both routes are
compared field by field.  Complete-run goldens only.
usage: mpfr_probe.py case[,case...]"""
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


class Mpz(C.Structure):
    _fields_ = [("alloc", C.c_int), ("size", C.c_int), ("d", C.c_void_p)]


class Mpq(C.Structure):
    _fields_ = [("num", Mpz), ("den", Mpz)]


class Mpfr(C.Structure):                                    # __mpfr_struct
    _fields_ = [("prec", C.c_long), ("sign", C.c_int), ("exp", C.c_long), ("d", C.POINTER(C.c_uint64))]


GMP = C.CDLL(ctypes.util.find_library("gmp") or "libgmp.so.10", mode=C.RTLD_GLOBAL)
MPFR = C.CDLL(ctypes.util.find_library("mpfr") or "libmpfr.so.6")
GMP.__gmpz_set_str.argtypes = [C.POINTER(Mpz), C.c_char_p, C.c_int]
GMP.__gmpq_init.argtypes = [C.POINTER(Mpq)]
GMP.__gmpq_clear.argtypes = [C.POINTER(Mpq)]
MPFR.mpfr_init2.argtypes = [C.POINTER(Mpfr), C.c_long]
MPFR.mpfr_init2.restype = None
MPFR.mpfr_set_q.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
MPFR.mpfr_clear.argtypes = [C.POINTER(Mpfr)]
MPFR.mpfr_clear.restype = None
EXP_ZERO = -(2 ** 63) + 1


def wall(fn):
    t = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t) * 1e3


def host_set_q(fracs, prec, rnd):
    """([(sign, exp, limbs)] as mpfr_set_q leaves them, ms of the mpfr_set_q calls alone)"""
    qs, xs = (Mpq * len(fracs))(), (Mpfr * len(fracs))()
    for q, x, (N, D) in zip(qs, xs, fracs):
        GMP.__gmpq_init(C.byref(q))
        GMP.__gmpz_set_str(C.byref(q.num), format(N, "x").encode(), 16)
        GMP.__gmpz_set_str(C.byref(q.den), format(D, "x").encode(), 16)
        MPFR.mpfr_init2(C.byref(x), prec)
    refs = [(C.addressof(x), C.addressof(q)) for q, x in zip(qs, xs)]
    set_q = MPFR.mpfr_set_q
    t = time.perf_counter()
    for xr, qr in refs:
        set_q(xr, qr, rnd)
    ms = (time.perf_counter() - t) * 1e3
    nl = (prec + 63) // 64
    out = [(0, 0, [0] * nl) if x.exp == EXP_ZERO else (1 if x.sign > 0 else -1, int(x.exp), [int(x.d[k]) for k in range(nl)]) for x in xs]
    for q, x in zip(qs, xs):
        GMP.__gmpq_clear(C.byref(q)); MPFR.mpfr_clear(C.byref(x))
    return out, ms


for name in [c for c in (sys.argv[1] if len(sys.argv) > 1 else "").split(",") if c]:
    e, fx = load_case(name)
    n, q = e["n"], np.asarray(fx["q"])
    g = sl.Factorization(n, fx["Ap"], fx["Ai"], fx["Alen"], fx["Alimbs"], q, pivot=e["pivot"], tol=e["tol"])
    g.run(0)
    det = oracle_lib.bigints(*g.pivots())[-1]
    b = (np.arange(n, dtype=np.int64) * 2654435761 % (1 << 32)) % 2001 - 1000
    bl, bx = sl.ints_to_slab(b)
    for nrhs in (1, 16):
        cl, cx = np.tile(bl, nrhs), np.tile(bx, nrhs)
        g.solve_rational(cl, cx, nrhs=nrhs)
        (numlen, numl, denlen, denl), rwall = wall(lambda: g.solve_rational(cl, cx, nrhs=nrhs))
        red_ms = g.to_rational_ms()
        fracs = list(zip(oracle_lib.bigints(numlen[:n], numl), oracle_lib.bigints(denlen[:n], denl)))      # the first right-hand side
        for prec in (53, 128, 1000):
            g.solve_mpfr(cl, cx, nrhs=nrhs, prec=prec)
            (sign, exp, mant, tern), mwall = wall(lambda: g.solve_mpfr(cl, cx, nrhs=nrhs, prec=prec))
            solve_ms, conv_ms, paths = g.solve_ms(), g.to_mpfr_ms(), g.to_mpfr_paths()
            want, setq_ms = host_set_q(fracs, prec, 0)
            same = all((int(sign[j]), int(exp[j]), [int(v) for v in mant[j]]) == want[j] for j in range(n))
            print(json.dumps(dict(case=name, n=n, nrhs=nrhs, prec=prec, det_limbs=(det.bit_length() + 63) // 64,
                                  solve_ms=round(solve_ms, 3), to_mpfr_ms=round(conv_ms, 3), to_rational_ms=round(red_ms, 3),
                                  paths=[round(v / (n * nrhs), 4) for v in paths], mpfr_wall_ms=round(mwall, 2),
                                  rational_wall_ms=round(rwall, 2), set_q_ms=round(setq_ms * nrhs, 2),
                                  d2h_mpfr=int(sign.nbytes + exp.nbytes + mant.nbytes + tern.nbytes),
                                  d2h_rational=int(4 * (numlen.size + denlen.size) + 8 * (numl.size + denl.size)), identical=same)),
                  flush=True)
    g.close()
