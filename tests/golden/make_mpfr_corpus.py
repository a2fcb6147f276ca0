#!/usr/bin/env python3
"""Generate tests/golden/mpfr_corpus.json.gz: rationals N / D and what MPFR's mpfr_set_q leaves for each in an mpfr_t of a given
precision under each of the five rounding modes.

mpfr_set_q is what SLIP_get_mpfr_soln calls per entry of a solution: the correct rounding of the exact quotient to `prec` bits.
This script asks the system libmpfr and libgmp (ctypes, no header, nothing of the reference): mpfr_init2, mpfr_set_q, and the
four fields of __mpfr_struct (precision, sign, exponent, limbs).  The corpus pins slip_mpfr_kernel and
tests/mpfr_helpers.py:round_mpfr to MPFR itself.  Deterministic: one seeded random.Random, no time, no environment.

Layout: NDEN denominators; per denominator GENERIC numerators (the same for every precision) and, per precision p, the SHAPES
built around p (the kernel test runs one (precision, mode) as one call with n = numerators per denominator and nrhs =
denominators).  Precision 8300 (more than 256 digits of 32 bits) is recorded for the two denominators above 8192 bits only,
and for a few of the numerators (GSEL_WIDE, SSEL_WIDE): 260 quotient digits each make them the slow ones in the emulator.

A numerator is stored once, as [s, m, r] with N = s * (m * |D| + r), m and r in hex: the structured shapes are a multiple of D
plus a little, so this keeps the file small.  A result is stored per (denominator, precision, numerator) as
{"m": [distinct mantissas in hex, as integers 2^(p-1) <= m < 2^p], "v": [[sign, exp, index into m, ternary] per mode 0..4]};
a zero is [0, 0, -1, 0].

JSON: {"den": [hex], "prec": [..], "prec_den": [[indices of den] per precision], "generic": [name], "shapes": [name],
"gsel", "ssel": [[indices of generic / shapes used] per precision], "pad": [[high zero limbs to append in the slab, per
numerator of a row] per precision], "num": [[..] per den], "pnum": [[[..] per precision] per den],
"res": [[[..per numerator] per precision] per den]}.  A row is the selected generic numerators, then the selected shapes.

Usage:  python tests/golden/make_mpfr_corpus.py
"""
import ctypes as C
import ctypes.util
import gzip
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "mpfr_corpus.json.gz")

PRECS = [2, 24, 53, 64, 65, 128, 200, 1000, 8300]
MODES = 5                                                   # MPFR_RNDN, RNDZ, RNDU, RNDD, RNDA


class Mpz(C.Structure):
    _fields_ = [("alloc", C.c_int), ("size", C.c_int), ("d", C.c_void_p)]


class Mpq(C.Structure):
    _fields_ = [("num", Mpz), ("den", Mpz)]


class Mpfr(C.Structure):                                    # __mpfr_struct
    _fields_ = [("prec", C.c_long), ("sign", C.c_int), ("exp", C.c_long), ("d", C.POINTER(C.c_uint64))]


def libraries():
    gmp = C.CDLL(ctypes.util.find_library("gmp") or "libgmp.so.10", mode=C.RTLD_GLOBAL)
    mpfr = C.CDLL(ctypes.util.find_library("mpfr") or "libmpfr.so.6")
    gmp.__gmpz_set_str.argtypes = [C.POINTER(Mpz), C.c_char_p, C.c_int]
    gmp.__gmpq_init.argtypes = [C.POINTER(Mpq)]
    gmp.__gmpq_clear.argtypes = [C.POINTER(Mpq)]
    mpfr.mpfr_init2.argtypes = [C.POINTER(Mpfr), C.c_long]
    mpfr.mpfr_init2.restype = None
    mpfr.mpfr_set_q.argtypes = [C.POINTER(Mpfr), C.POINTER(Mpq), C.c_int]
    mpfr.mpfr_set_q.restype = C.c_int
    mpfr.mpfr_clear.argtypes = [C.POINTER(Mpfr)]
    mpfr.mpfr_clear.restype = None
    return gmp, mpfr


EXP_ZERO = -(2 ** 63) + 1                                   # __MPFR_EXP_ZERO


def mpfr_set_q(libs, num, den, prec, rnd):
    """MPFR's answer for num / den (den != 0): (sign, exp, m, ternary) with the mantissa as an integer of exactly prec bits"""
    gmp, mpfr = libs
    if den < 0:
        num, den = -num, -den
    q, x = Mpq(), Mpfr()
    gmp.__gmpq_init(C.byref(q))
    assert gmp.__gmpz_set_str(C.byref(q.num), format(num, "x").encode(), 16) == 0
    assert gmp.__gmpz_set_str(C.byref(q.den), format(den, "x").encode(), 16) == 0
    mpfr.mpfr_init2(C.byref(x), prec)
    t = mpfr.mpfr_set_q(C.byref(x), C.byref(q), rnd)
    t = (t > 0) - (t < 0)
    assert x.prec == prec
    if x.exp == EXP_ZERO:
        out = (0, 0, 0, t)
        assert x.sign > 0                                   # a zero quotient is +0 under every mode
    else:
        nl = (prec + 63) // 64
        image = sum(int(x.d[k]) << (64 * k) for k in range(nl))
        z = 64 * nl - prec
        assert image >> (64 * nl - 1) == 1 and image & ((1 << z) - 1) == 0
        out = (1 if x.sign > 0 else -1, int(x.exp), image >> z, t)
    mpfr.mpfr_clear(C.byref(x))
    gmp.__gmpq_clear(C.byref(q))
    return out


def rand_bits(rng, bits):
    """a random integer of exactly `bits` bits"""
    return (1 << (bits - 1)) | rng.getrandbits(bits - 1) if bits > 1 else 1


GENERIC = ["zero", "random near", "random large negative", "|N| << |D|", "|N| >> |D|", "-(m*D << 2200)", "(m*D << 2200) + 1",
           "random, 2 high zero limbs", "2^64 - 1", "one", "minus three"]
SHAPES = ["M*D", "M*D+1", "M*D-1", "tie, M even", "tie, M odd", "tie even +1", "tie even -1", "tie odd +1", "tie odd -1",
          "all ones", "2^k*D", "2^k*D-1", "-M*D", "-(tie, M odd)", "-(tie even + 1)", "-(all ones)", "M*D, 1 high zero limb"]


GSEL_WIDE = ["zero", "random near"]
SSEL_WIDE = ["M*D+1", "tie, M odd", "all ones", "-(tie even + 1)"]


def generic(rng, D):
    """[(N, high zero limbs)] in the order of GENERIC"""
    a, bd = abs(D), abs(D).bit_length()
    m = rand_bits(rng, 60)
    return [(0, 0),
            (rand_bits(rng, max(1, bd + rng.randrange(-60, 61))), 0),
            (-rand_bits(rng, bd + 200), 0),
            (rand_bits(rng, bd - 2100) if bd > 2100 else 1, 0),
            (rand_bits(rng, bd + 2100), 0),
            (-((m * a) << 2200), 0), (((m * a) << 2200) + 1, 0),
            (rand_bits(rng, bd + 17), 2), (2 ** 64 - 1, 0), (1, 0), (-3, 0)]


def shaped(rng, D, p):
    """[(N, high zero limbs)] in the order of SHAPES, for the precision p"""
    a = abs(D)
    M = rand_bits(rng, p)
    Me, Mo = M & ~1, M | 1                                  # exactly p bits both (p >= 2)
    te, to = (2 * Me + 1) * a, (2 * Mo + 1) * a             # N / D = 2M + 1: p + 1 bits, the last one set -- an exact tie
    ones = ((1 << p) - 1) * a + (a - 1)
    k = rng.randrange(0, 200)
    return [(M * a, 0), (M * a + 1, 0), (M * a - 1, 0), (te, 0), (to, 0), (te + 1, 0), (te - 1, 0), (to + 1, 0), (to - 1, 0),
            (ones, 0), (a << k, 0), ((a << k) - 1, 0), (-(M * a), 0), (-to, 0), (-(te + 1), 0), (-ones, 0),
            (rand_bits(rng, p) * a, 1)]


def denominators(rng):
    return [1, 3, 10, rand_bits(rng, 64), rand_bits(rng, 65), rand_bits(rng, 1000), 1 << 63, 1 << 1000, -rand_bits(rng, 128),
            rand_bits(rng, 3000), rand_bits(rng, 8200), -rand_bits(rng, 9001)]


def stored(N, D):
    a = abs(D)
    m, r = divmod(abs(N), a)
    return [-1 if N < 0 else 1, format(m, "x"), format(r, "x")]


def main():
    rng = random.Random(20250611)
    libs = libraries()
    dens = denominators(rng)
    prec_den = [[c for c, D in enumerate(dens) if p != 8300 or abs(D).bit_length() > 8192] for p in PRECS]
    gsel = [[t for t, nm in enumerate(GENERIC) if p != 8300 or nm in GSEL_WIDE] for p in PRECS]
    ssel = [[t for t, nm in enumerate(SHAPES) if p != 8300 or nm in SSEL_WIDE] for p in PRECS]
    num, pnum, pad, res = [], [], [None] * len(PRECS), []
    for c, D in enumerate(dens):
        g = generic(rng, D)
        num.append([stored(N, D) for N, _ in g])
        rows, rres = [], []
        for pi, p in enumerate(PRECS):
            if c not in prec_den[pi]:
                rows.append([]); rres.append([])
                continue
            s = shaped(rng, D, p)
            assert len(g) == len(GENERIC) and len(s) == len(SHAPES)
            row = [g[t] for t in gsel[pi]] + [s[t] for t in ssel[pi]]
            rows.append([stored(N, D) for N, _ in row[len(gsel[pi]):]])
            row_pad = [q for _, q in row]
            assert pad[pi] is None or pad[pi] == row_pad
            pad[pi] = row_pad
            out = []
            for N, _ in row:
                got = [mpfr_set_q(libs, N, D, p, rnd) for rnd in range(MODES)]
                mants = sorted({m for sg, _, m, _ in got if sg})
                out.append({"m": [format(m, "x") for m in mants],
                            "v": [[sg, e, mants.index(m) if sg else -1, t] for sg, e, m, t in got]})
            rres.append(out)
        pnum.append(rows); res.append(rres)
    doc = {"den": [format(D, "x") for D in dens], "prec": PRECS, "prec_den": prec_den, "generic": GENERIC, "shapes": SHAPES,
           "gsel": gsel, "ssel": ssel, "pad": pad, "num": num, "pnum": pnum, "res": res}
    raw = json.dumps(doc, separators=(",", ":")).encode()
    with open(OUT, "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as g:
            g.write(raw)
    print(f"{OUT}: {len(dens)} denominators x {len(PRECS)} precisions x up to {len(GENERIC) + len(SHAPES)} numerators x {MODES} modes, "
          f"{os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
