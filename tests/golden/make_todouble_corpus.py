#!/usr/bin/env python3
"""Generate tests/golden/todouble_corpus.json.gz: rationals N / D and the 8 bytes GMP's mpq_get_d returns for each.

mpq_get_d is what SLIP_get_double_soln calls per entry of a solution; it truncates the exact quotient toward zero onto the
double grid.  This script asks the system libgmp (ctypes, no header, nothing of the reference) and records its answer, so the
corpus pins slip_todouble_kernel and tests/todouble_helpers.py:trunc_double to GMP itself.  Deterministic: one seeded
random.Random, no time, no environment.

Layout: NDEN denominators, for each the same NNUM numerator shapes (the kernel test runs the whole corpus as one call with
n = NNUM and nrhs = NDEN).  Denominators: 1, 53, 64, 65, 128 and 1000 bits, powers of two (among them 2^1074, 2^1075 and 2^1080
for the subnormal and underflow cases), two of about 3000 bits, two above 8192 bits (more than 256 digits: the kernel's
memory path), a few negative ones (the sign is carried).  Numerator shapes: see SHAPES.  GMP wants a positive denominator: a
negative one hands its sign to the numerator before the call.

JSON: {"den": [hex], "shapes": [name], "num": [[hex]], "pad": [[high zero limbs to append in the slab]], "bits": [[16 hex
digits: struct.pack('>d', result)]]}.

Usage:  python tests/golden/make_todouble_corpus.py
"""
import ctypes as C
import ctypes.util
import gzip
import json
import os
import random
import struct

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "todouble_corpus.json.gz")


class Mpz(C.Structure):
    _fields_ = [("alloc", C.c_int), ("size", C.c_int), ("d", C.c_void_p)]


class Mpq(C.Structure):
    _fields_ = [("num", Mpz), ("den", Mpz)]


def gmp():
    lib = C.CDLL(ctypes.util.find_library("gmp") or "libgmp.so.10")
    lib.__gmpq_get_d.restype = C.c_double
    lib.__gmpq_get_d.argtypes = [C.POINTER(Mpq)]
    lib.__gmpz_set_str.argtypes = [C.POINTER(Mpz), C.c_char_p, C.c_int]
    lib.__gmpq_init.argtypes = [C.POINTER(Mpq)]
    lib.__gmpq_clear.argtypes = [C.POINTER(Mpq)]
    return lib


def mpq_get_d(lib, num, den):
    """GMP's answer for num / den (den != 0; not canonicalised: mpq_get_d does not need lowest terms)"""
    if den < 0:
        num, den = -num, -den
    q = Mpq()
    lib.__gmpq_init(C.byref(q))
    assert lib.__gmpz_set_str(C.byref(q.num), format(num, "x").encode(), 16) == 0
    assert lib.__gmpz_set_str(C.byref(q.den), format(den, "x").encode(), 16) == 0
    v = lib.__gmpq_get_d(C.byref(q))
    lib.__gmpq_clear(C.byref(q))
    return v


def rand_bits(rng, bits):
    """a random integer of exactly `bits` bits"""
    return (1 << (bits - 1)) | rng.getrandbits(bits - 1) if bits > 1 else 1


SHAPES = ["zero", "random near", "random large negative", "random small", "m*D", "m*D+1", "m*D-1", "-m*D odd m", "-(m*D+1)",
          "-(m*D-1)", "2^k*D", "2^k*D-1", "(2^54-1)*D", "3*D", "(2^1024-1)*D", "2^1024*D", "-2^1030*D", "2^1024*D-1",
          "D>>1060 or 1", "-(D>>1075|1)", "(D>>1022)+1", "random, 2 high zero limbs", "m*D, 1 high zero limb", "one", "minus three"]


def numerators(rng, D):
    """[(N, high zero limbs)] in the order of SHAPES, for the denominator D"""
    a, bd = abs(D), abs(D).bit_length()
    m = rand_bits(rng, 53)
    mo = rand_bits(rng, 53) | 1
    k = rng.randrange(0, 200)
    out = [(0, 0),
           (rand_bits(rng, max(1, bd + rng.randrange(-60, 61))), 0),
           (-rand_bits(rng, bd + 200), 0),
           (rand_bits(rng, max(1, bd - 300)), 0),
           (m * a, 0), (m * a + 1, 0), (m * a - 1, 0), (-mo * a, 0), (-(mo * a + 1), 0), (-(mo * a - 1), 0),
           ((a << k), 0), ((a << k) - 1, 0), (((1 << 54) - 1) * a, 0), (3 * a, 0),
           (((1 << 1024) - 1) * a, 0), (a << 1024, 0), (-(a << 1030), 0), ((a << 1024) - 1, 0),
           ((a >> 1060) or 1, 0), (-((a >> 1075) | 1), 0), ((a >> 1022) + 1, 0),
           (rand_bits(rng, bd + 17), 2), (rand_bits(rng, 53) * a, 1), (1, 0), (-3, 0)]
    assert len(out) == len(SHAPES)
    return out


def denominators(rng):
    dens = [1, 3, 10, rand_bits(rng, 53), rand_bits(rng, 64), -rand_bits(rng, 64), rand_bits(rng, 65), rand_bits(rng, 128),
            rand_bits(rng, 1000), -(rand_bits(rng, 1000) | 1),
            2, 1 << 52, 1 << 63, 1 << 64, 1 << 1000, 1 << 1022, 1 << 1074, 1 << 1075, -(1 << 1075), 1 << 1080,
            7 << 60, rand_bits(rng, 3000), rand_bits(rng, 2999) | 1, rand_bits(rng, 8200), -rand_bits(rng, 9001)]
    return dens


def main():
    rng = random.Random(20250117)
    lib = gmp()
    dens = denominators(rng)
    num, pad, bits = [], [], []
    for D in dens:
        row = numerators(rng, D)
        num.append([format(N, "x") for N, _ in row])
        pad.append([p for _, p in row])
        bits.append([struct.pack(">d", mpq_get_d(lib, N, D)).hex() for N, _ in row])
    doc = {"den": [format(D, "x") for D in dens], "shapes": SHAPES, "num": num, "pad": pad, "bits": bits}
    raw = json.dumps(doc, separators=(",", ":")).encode()
    with open(OUT, "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as g:
            g.write(raw)
    print(f"{OUT}: {len(dens)} denominators x {len(SHAPES)} numerators, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
