"""The drop-in SLIP_solve_mpfr (libslip_lu_hip.so: SLIP_hip_solve_mpfr, also exported under the reference's name): a caller that
holds GMP-typed SLIP_sparse / SLIP_LU_analysis / SLIP_dense and an initialised mpfr_t matrix gets its correctly rounded floats
from the device.  The structures are laid out here with ctypes exactly as include/SLIP_LU_hip.h mirrors them, their mpz_t and
mpfr_t initialised by the system libgmp and libmpfr; the result is read back from the mpfr_t fields themselves: sign, exponent,
limbs.  Nothing of the reference is compiled or loaded."""
import ctypes as C
import ctypes.util
import json
import os

import pytest

import oracle_lib
from check_helpers import slab
from conftest import GOLDEN, ROOT, solve_inputs
from mpfr_helpers import MODES, RNDN, limbs_of, round_mpfr
from todouble_helpers import rhs_pattern

pytestmark = pytest.mark.gpu
SOLVE_CASES = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "solve_index.json")))}
SHIM = os.path.join(ROOT, "slip_lu_amd", "csrc", "libslip_lu_hip.so")
SLIP_OK, SLIP_INCORRECT_INPUT = 0, -3
EXP_ZERO = -(2 ** 63) + 1                    # __MPFR_EXP_ZERO


class Mpz(C.Structure):
    _fields_ = [("alloc", C.c_int), ("size", C.c_int), ("d", C.c_void_p)]


class Mpq(C.Structure):
    _fields_ = [("num", Mpz), ("den", Mpz)]


class Mpfr(C.Structure):                     # __mpfr_struct
    _fields_ = [("prec", C.c_long), ("sign", C.c_int), ("exp", C.c_long), ("d", C.POINTER(C.c_uint64))]


class Sparse(C.Structure):                   # SLIP_sparse
    _fields_ = [("m", C.c_int32), ("n", C.c_int32), ("nzmax", C.c_int32), ("nz", C.c_int32),
                ("p", C.POINTER(C.c_int32)), ("i", C.POINTER(C.c_int32)), ("x", C.POINTER(Mpz)), ("scale", Mpq)]


class Analysis(C.Structure):                 # SLIP_LU_analysis
    _fields_ = [("q", C.POINTER(C.c_int32)), ("lnz", C.c_int32), ("unz", C.c_int32)]


class Dense(C.Structure):                    # SLIP_dense
    _fields_ = [("m", C.c_int32), ("n", C.c_int32), ("x", C.POINTER(C.POINTER(Mpz))), ("scale", Mpq)]


class Options(C.Structure):                  # SLIP_options
    _fields_ = [("pivot", C.c_int32), ("order", C.c_int32), ("tol", C.c_double), ("print_level", C.c_int32),
                ("prec", C.c_uint64), ("SLIP_MPFR_ROUND", C.c_int32)]


@pytest.fixture(scope="module")
def libs():
    assert os.path.exists(SHIM), "libslip_lu_hip.so missing: __graft_entry__.build() makes it where gmp.h is"
    gmp = C.CDLL(ctypes.util.find_library("gmp") or "libgmp.so.10", mode=C.RTLD_GLOBAL)
    getattr(gmp, "__gmpz_init_set_str").argtypes = [C.POINTER(Mpz), C.c_char_p, C.c_int]
    getattr(gmp, "__gmpz_clear").argtypes = [C.POINTER(Mpz)]
    shim = C.CDLL(SHIM)
    if not hasattr(shim, "SLIP_hip_solve_mpfr"):
        pytest.skip("libslip_lu_hip.so was built without mpfr.h: it holds no SLIP_solve_mpfr")
    mpfr = C.CDLL(ctypes.util.find_library("mpfr") or "libmpfr.so.6", mode=C.RTLD_GLOBAL)
    mpfr.mpfr_init2.argtypes = [C.POINTER(Mpfr), C.c_long]
    mpfr.mpfr_init2.restype = None
    mpfr.mpfr_clear.argtypes = [C.POINTER(Mpfr)]
    mpfr.mpfr_clear.restype = None
    mpfr.mpfr_set_si.argtypes = [C.POINTER(Mpfr), C.c_long, C.c_int]
    for fn in (shim.SLIP_hip_solve_mpfr, shim.SLIP_solve_mpfr):
        fn.argtypes = [C.c_void_p] * 5
        fn.restype = C.c_int
    return gmp, mpfr, shim


class Problem:
    """A, S, b and x_mpfr of one call, kept alive together; every mpz_t comes from GMP, every mpfr_t from MPFR, and goes back"""

    def __init__(self, gmp, mpfr, n, Ap, Ai, vals, q, bs, a_scale, b_scale, prec, rnd):
        self.gmp, self.mpfr, self.n, self.nrhs, self.z, self.prec = gmp, mpfr, n, len(bs), [], prec
        nz = len(vals)
        self.Ap = (C.c_int32 * (n + 1))(*[int(v) for v in Ap]); self.Ai = (C.c_int32 * nz)(*[int(v) for v in Ai])
        self.Ax = (Mpz * nz)()
        for t, v in enumerate(vals):
            self.set(self.Ax[t], v)
        self.A = Sparse(n, n, nz, nz, self.Ap, self.Ai, self.Ax)
        self.set(self.A.scale.num, a_scale[0]); self.set(self.A.scale.den, a_scale[1])
        self.q = (C.c_int32 * n)(*[int(v) for v in q])
        self.S = Analysis(self.q, 0, 0)
        self.rows = [(Mpz * self.nrhs)() for _ in range(n)]
        for i in range(n):
            for k in range(self.nrhs):
                self.set(self.rows[i][k], bs[k][i])
        self.bx = (C.POINTER(Mpz) * n)(*[C.cast(r, C.POINTER(Mpz)) for r in self.rows])
        self.b = Dense(n, self.nrhs, self.bx)
        self.set(self.b.scale.num, b_scale[0]); self.set(self.b.scale.den, b_scale[1])
        self.opt = Options(3, 0, 1.0, 0, prec, rnd)                               # SLIP_TOL_SMALLEST, tol 1: the defaults
        self.xrows = [(Mpfr * self.nrhs)() for _ in range(n)]                     # as SLIP_create_mpfr_mat: every entry option->prec
        for r in self.xrows:
            for k in range(self.nrhs):
                mpfr.mpfr_init2(C.byref(r[k]), prec)
        self.x = (C.POINTER(Mpfr) * n)(*[C.cast(r, C.POINTER(Mpfr)) for r in self.xrows])

    def set(self, z, v):
        assert getattr(self.gmp, "__gmpz_init_set_str")(C.byref(z), format(int(v), "x").encode(), 16) == 0    # (no name mangling)
        self.z.append(z)

    def args(self):
        return [C.addressof(self.x), C.addressof(self.A), C.addressof(self.S), C.addressof(self.b), C.addressof(self.opt)]

    def poison(self):
        for r in self.xrows:
            for k in range(self.nrhs):
                self.mpfr.mpfr_set_si(C.byref(r[k]), -77, 0)

    def read(self, i, k):
        """(sign, exp, limbs) of x_mpfr[i][k] from the fields of the mpfr_t; a zero is (0, 0, all-zero limbs), +0 only"""
        x = self.xrows[i][k]
        nl = (self.prec + 63) // 64
        assert x.prec == self.prec
        if x.exp == EXP_ZERO:
            assert x.sign > 0, "a negative zero"
            return 0, 0, [0] * nl
        return (1 if x.sign > 0 else -1), int(x.exp), [int(x.d[t]) for t in range(nl)]

    def close(self):
        for z in self.z:
            getattr(self.gmp, "__gmpz_clear")(C.byref(z))
        self.z = []
        for r in self.xrows:
            for k in range(self.nrhs):
                self.mpfr.mpfr_clear(C.byref(r[k]))
        self.xrows = []


@pytest.mark.parametrize("name", ["solve_test_mat", "solve_10teams"])
@pytest.mark.parametrize("prec", [128, 53])
def test_dropin_solve_mpfr(libs, name, prec):
    """A->scale = 1000, b->scale = 7/3: x = round(1000 / (7/3) * xnum / xden), one rounding of the exact value, for the
    reference's own rationals of the first right-hand side and a handle's numerators of the second; both exported names;
    nearest under one name, toward minus infinity under the other"""
    import slip_lu_amd as sl
    gmp, mpfr, shim = libs
    n, Ap, Ai, Alen, Alimbs, q, fix = solve_inputs(SOLVE_CASES[name])
    num = oracle_lib.bigints(fix["xnumlen"], fix["xnumlimbs"])
    den = oracle_lib.bigints(fix["xdenlen"], fix["xdenlimbs"])
    bs = rhs_pattern(oracle_lib.solve_rhs(n), 2)
    f = sl.Factorization(n, Ap, Ai, Alen, Alimbs, q)
    try:
        f.run(0)
        det = oracle_lib.bigints(*f.pivots())[-1]
        x = oracle_lib.bigints(*f.solve(*slab([v for b in bs for v in b]), nrhs=2))
    finally:
        f.close()
    for fn, rnd in ((shim.SLIP_hip_solve_mpfr, RNDN), (shim.SLIP_solve_mpfr, MODES[3])):
        pr = Problem(gmp, mpfr, n, Ap, Ai, oracle_lib.bigints(Alen, Alimbs), q, bs, (1000, 1), (7, 3), prec, rnd)
        try:
            pr.poison()
            assert fn(*pr.args()) == SLIP_OK
            bad = []
            for p in range(n):
                i = int(q[p])
                for k, (N, D) in enumerate(((num[p] * 3000, den[p] * 7), (x[n + p] * 3000, det * 7))):
                    s, e, m, _ = round_mpfr(N, D, prec, rnd)
                    if pr.read(i, k) != (s, e, limbs_of(m, prec)):
                        bad.append((i, k, pr.read(i, k), (s, e, limbs_of(m, prec))))
            assert not bad, (name, prec, rnd, len(bad), bad[:3])
        finally:
            pr.close()


def test_dropin_solve_mpfr_rejects_bad_arguments(libs):
    """SLIP_solve_mpfr.c:52-56: any missing argument or array is SLIP_INCORRECT_INPUT; so are entries of differing precisions
    (the documented difference from the reference) and a rounding mode MPFR's set_q does not take"""
    gmp, mpfr, shim = libs
    n, Ap, Ai, Alen, Alimbs, q, _ = solve_inputs(SOLVE_CASES["solve_test_mat"])
    pr = Problem(gmp, mpfr, n, Ap, Ai, oracle_lib.bigints(Alen, Alimbs), q, rhs_pattern(oracle_lib.solve_rhs(n), 1), (1, 1), (1, 1), 128, RNDN)
    try:
        good = pr.args()
        for k in range(5):
            assert shim.SLIP_hip_solve_mpfr(*[None if t == k else a for t, a in enumerate(good)]) == SLIP_INCORRECT_INPUT, k
        for obj, field in ((pr.A, "p"), (pr.A, "i"), (pr.A, "x"), (pr.S, "q"), (pr.b, "x")):
            ptr = getattr(obj, field)                                 # a view of the field itself: keep the address, not the view
            addr = C.cast(ptr, C.c_void_p).value
            setattr(obj, field, type(ptr)())
            assert shim.SLIP_hip_solve_mpfr(*good) == SLIP_INCORRECT_INPUT, field
            setattr(obj, field, C.cast(addr, type(ptr)))
        assert shim.SLIP_hip_solve_mpfr(*good) == SLIP_OK
        pr.opt.SLIP_MPFR_ROUND = 5                                    # MPFR_RNDF
        assert shim.SLIP_hip_solve_mpfr(*good) == SLIP_INCORRECT_INPUT
        pr.opt.SLIP_MPFR_ROUND = 0
        odd = pr.xrows[n - 1][0]
        mpfr.mpfr_clear(C.byref(odd)); mpfr.mpfr_init2(C.byref(odd), 64)     # one entry of another precision
        assert shim.SLIP_hip_solve_mpfr(*good) == SLIP_INCORRECT_INPUT
        assert shim.SLIP_solve_mpfr(*good) == SLIP_INCORRECT_INPUT
    finally:
        pr.close()
