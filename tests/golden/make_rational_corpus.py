#!/usr/bin/env python3
"""Generate tests/golden/rational_corpus.json.gz: rationals N / D and the canonical form GMP's mpq_canonicalize leaves of each.

Every mpq_* call of SLIP_solve_mpq's tail (mpq_div, SLIP_permute_x, SLIP_scale_x) canonicalises its result: lowest terms, a
positive denominator, 0 as 0 / 1.  This script asks the system libgmp (ctypes, no header, nothing of the reference) and records
its answer, so the corpus pins slip_reduce_kernel and tests/rational_helpers.py:canonical to GMP itself.  Deterministic: one
seeded random.Random, no time, no environment.

Layout: NDEN denominators, for each the same NNUM numerator shapes (the kernel test runs the whole corpus as one call with
n = NNUM and nrhs = NDEN).  A denominator is built as a product of planted factors -- an odd factor of 32, 64 and 40 bits, one of
half its bits, for some a power of two -- so that every shape that needs a common factor of a given size exists for it (small
denominators take the nearest divisor they have).  Sizes: 1, 32, 33, 64 and 65 bits, 2^32 and 2^64 themselves (the boundary
between the kernel's lane and wave passes), 64*32, 64*32+1, 128*32, 128*32+1 and 256*32 bits (the register classes' edges),
257*32 and about 9000 bits (the memory class), a power of two, an odd number times 2^70, two negative ones, and two of the
form h * F(k) for the Fibonacci shape.  Numerator shapes: see SHAPES.

JSON: {"den": [hex], "shapes": [name], "num": [[hex]], "pad": [[high zero limbs to append in the slab]], "dpad": [the same per
denominator], "cnum": [[hex]], "cden": [[hex]]}.

Usage:  python tests/golden/make_rational_corpus.py
"""
import ctypes as C
import ctypes.util
import gzip
import json
import math
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "rational_corpus.json.gz")


class Mpz(C.Structure):
    _fields_ = [("alloc", C.c_int), ("size", C.c_int), ("d", C.c_void_p)]


class Mpq(C.Structure):
    _fields_ = [("num", Mpz), ("den", Mpz)]


def gmp():
    lib = C.CDLL(ctypes.util.find_library("gmp") or "libgmp.so.10")
    lib.__gmpq_canonicalize.argtypes = [C.POINTER(Mpq)]
    lib.__gmpz_set_str.argtypes = [C.POINTER(Mpz), C.c_char_p, C.c_int]
    lib.__gmpz_get_str.argtypes = [C.c_char_p, C.c_int, C.POINTER(Mpz)]
    lib.__gmpz_get_str.restype = C.c_char_p
    lib.__gmpz_sizeinbase.argtypes = [C.POINTER(Mpz), C.c_int]
    lib.__gmpz_sizeinbase.restype = C.c_size_t
    lib.__gmpq_init.argtypes = [C.POINTER(Mpq)]
    lib.__gmpq_clear.argtypes = [C.POINTER(Mpq)]
    return lib


def mpq_canonicalize(lib, num, den):
    """GMP's canonical (num, den) of num / den, den != 0"""
    q = Mpq()
    lib.__gmpq_init(C.byref(q))
    assert lib.__gmpz_set_str(C.byref(q.num), format(num, "x").encode(), 16) == 0
    assert lib.__gmpz_set_str(C.byref(q.den), format(den, "x").encode(), 16) == 0
    lib.__gmpq_canonicalize(C.byref(q))
    out = []
    for z in (q.num, q.den):
        buf = C.create_string_buffer(lib.__gmpz_sizeinbase(C.byref(z), 16) + 2)
        out.append(int(lib.__gmpz_get_str(buf, 16, C.byref(z)).decode(), 16))
    lib.__gmpq_clear(C.byref(q))
    return out[0], out[1]


def rand_bits(rng, bits):
    """a random integer of exactly `bits` bits"""
    return (1 << (bits - 1)) | rng.getrandbits(bits - 1) if bits > 1 else 1


def rand_odd(rng, bits):
    return rand_bits(rng, bits) | 1


def fib(k):
    a, b = 0, 1
    for _ in range(k):
        a, b = b, a + b
    return a, b                                              # F(k), F(k+1)


class Den:
    """a denominator with its planted factors: value = sign * 2^two * prod(odd)"""

    def __init__(self, odd, two=0, sign=1, fibk=0):
        self.odd, self.two, self.sign, self.fibk = list(odd), two, sign, fibk
        self.value = sign * (math.prod(odd) << two)

    def divisor(self, bits):
        """the odd planted divisor nearest to `bits` bits (greedy over the factors, largest first); 1 when there is none"""
        h = 1
        for f in sorted(self.odd, reverse=True):
            if (h * f).bit_length() <= bits + 1:
                h *= f
        return h


def planted(rng, bits, two=0, sign=1):
    """an exactly `bits`-bit denominator: 2^two times odd factors of 32, 64 and 40 bits, one of half the bits and a rest"""
    ob = bits - two
    if ob <= 65:
        sizes = [ob // 2, ob - ob // 2] if ob >= 4 else [ob]
    elif ob < 300:
        sizes = [32, 64, ob - 96]
    else:
        sizes = [32, 64, 40, ob // 2, ob - 136 - ob // 2]
    while True:
        d = Den([rand_odd(rng, s) for s in sizes], two, sign)
        if abs(d.value).bit_length() == bits:
            return d


def fib_den(rng, k, hbits):
    """h * F(k) for an odd h of about hbits bits that holds the planted factors too (F(k) odd: k is no multiple of 3)"""
    assert k % 3
    return Den([rand_odd(rng, 32), rand_odd(rng, 64), rand_odd(rng, 40), rand_odd(rng, hbits - 136), fib(k)[0]], fibk=k)


def denominators(rng):
    return [Den([1]), planted(rng, 32), planted(rng, 33), planted(rng, 64), planted(rng, 65), Den([1], two=32), Den([1], two=64),
            planted(rng, 64 * 32), planted(rng, 64 * 32 + 1, two=5), planted(rng, 128 * 32), planted(rng, 128 * 32 + 1),
            planted(rng, 256 * 32), planted(rng, 257 * 32, two=37), planted(rng, 9001),
            Den([1], two=200), planted(rng, 1000, two=70), planted(rng, 300, two=1, sign=-1), planted(rng, 700, sign=-1),
            fib_den(rng, 1000, 600), fib_den(rng, 6001, 4200)]


SHAPES = ["zero", "coprime, balanced", "coprime, 10x longer", "coprime, 10x shorter", "D", "-D", "m*D", "-D/f", "h=1", "h of 32 bits",
          "h of 64 bits", "h of half the bits", "h of all but 40 bits", "a power of two times coprime", "2^k * h * u", "one limb",
          "Fibonacci or golden partner", "h*u, 1 high zero limb", "h*u, 2 high zero limbs", "all-ones low digits", "-h*u", "3*h"]


def coprime(rng, bits, v):
    """a random odd `bits`-bit number coprime to v"""
    while True:
        u = rand_odd(rng, max(bits, 1))
        if math.gcd(u, v) == 1:
            return u


def numerators(rng, den):
    """[(N, high zero limbs)] in the order of SHAPES, for the denominator den"""
    D = den.value
    a, bd = abs(D), abs(D).bit_length()
    half, but40 = den.divisor(bd // 2), den.divisor(bd - 40)
    h32, h64 = den.divisor(32), den.divisor(64)
    f = min(den.odd)
    k = rng.randrange(1, 100)

    def hu(h, bits=None):
        v = a // h
        return h * coprime(rng, max((bits or bd) - h.bit_length(), 2), v)
    if den.fibk:
        fk, fk1 = fib(den.fibk)
        fibn = a // fk * fk1                                 # h * F(k+1) against h * F(k): every quotient is 1
    else:
        v = a // half
        fibn = half * ((v * 0x9E3779B97F4A7C15F39CC0605CEDC834) >> 128)      # v / phi: quotients of 1 while the precision lasts
    out = [(0, 0), (coprime(rng, bd, a), 0), (coprime(rng, 10 * bd, a), 0), (coprime(rng, max(bd // 10, 1), a), 0),
           (a, 0), (-a, 0), (rand_bits(rng, 53) * a, 0), (-(a // f), 0), (hu(1), 0), (hu(h32), 0), (hu(h64), 0), (hu(half), 0),
           (hu(but40), 0), (coprime(rng, bd, a) << k, 0), (hu(half) << k, 0),
           (h32 * coprime(rng, max(62 - h32.bit_length(), 2), a), 0), (fibn, 0), (hu(half, bd + 17), 1), (hu(but40), 2),
           ((rand_bits(rng, max(bd // 2, 1)) << (bd // 2 + 40)) | ((1 << (bd // 2 + 40)) - 1), 0), (-hu(half), 0), (3 * half, 0)]
    assert len(out) == len(SHAPES)
    return out


def main():
    rng = random.Random(20250211)
    lib = gmp()
    dens = denominators(rng)
    num, pad, cnum, cden = [], [], [], []
    total = reduced = big_odd = 0
    for den in dens:
        row = numerators(rng, den)
        num.append([format(N, "x") for N, _ in row])
        pad.append([p for _, p in row])
        ans = [mpq_canonicalize(lib, N, den.value) for N, _ in row]
        cnum.append([format(n, "x") for n, _ in ans])
        cden.append([format(d, "x") for _, d in ans])
        for (N, _), (_, d) in zip(row, ans):
            g = abs(den.value) // d
            total += 1
            reduced += g > 1
            big_odd += g & 1 and g.bit_length() > 64
    assert 2 * reduced >= total and 4 * big_odd >= total, (total, reduced, big_odd)
    doc = {"den": [format(d.value, "x") for d in dens], "dpad": [c % 2 for c in range(len(dens))], "shapes": SHAPES,
           "num": num, "pad": pad, "cnum": cnum, "cden": cden}
    raw = json.dumps(doc, separators=(",", ":")).encode()
    with open(OUT, "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as g:
            g.write(raw)
    print(f"{OUT}: {len(dens)} denominators x {len(SHAPES)} numerators, g > 1 for {reduced}, an odd g above 64 bits for "
          f"{big_odd} of {total}, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
