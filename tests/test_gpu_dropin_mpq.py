"""The drop-in SLIP_solve_mpq (libslip_lu_hip.so: SLIP_hip_solve_mpq, also exported under the reference's name): a caller that
holds GMP-typed SLIP_sparse / SLIP_LU_analysis / SLIP_dense gets its solution as canonical mpq_t from the device.  The structures
are laid out here with ctypes exactly as include/SLIP_LU_hip.h mirrors them, their mpz_t and mpq_t initialised by the system
libgmp; the result is read back from the mpq_t fields themselves, signs and limbs.  Nothing of the reference is compiled or
loaded."""
import ctypes as C
import ctypes.util
import json
import os

import pytest

import oracle_lib
from check_helpers import slab
from conftest import GOLDEN, ROOT, solve_inputs
from rational_helpers import assert_same_fractions, canonical, placed
from todouble_helpers import rhs_pattern

pytestmark = pytest.mark.gpu
SOLVE_CASES = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "solve_index.json")))}
SHIM = os.path.join(ROOT, "slip_lu_amd", "csrc", "libslip_lu_hip.so")
SLIP_OK, SLIP_INCORRECT_INPUT = 0, -3


class Mpz(C.Structure):
    _fields_ = [("alloc", C.c_int), ("size", C.c_int), ("d", C.c_void_p)]


class Mpq(C.Structure):
    _fields_ = [("num", Mpz), ("den", Mpz)]


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
    getattr(gmp, "__gmpq_init").argtypes = [C.POINTER(Mpq)]
    getattr(gmp, "__gmpq_clear").argtypes = [C.POINTER(Mpq)]
    shim = C.CDLL(SHIM)
    for fn in (shim.SLIP_hip_solve_mpq, shim.SLIP_solve_mpq):
        fn.argtypes = [C.c_void_p] * 5
        fn.restype = C.c_int
    return gmp, shim


def mpz_value(z):
    """the integer behind an mpz_t, from its fields: _mp_size signed limbs at _mp_d, no high zero limb"""
    l = abs(z.size)
    limbs = C.cast(z.d, C.POINTER(C.c_uint64))
    assert l == 0 or limbs[l - 1] != 0, "a high zero limb"
    v = sum(int(limbs[t]) << (64 * t) for t in range(l))
    return -v if z.size < 0 else v


class Problem:
    """A, S, b and x_mpq of one call, kept alive together; every mpz_t and mpq_t comes from GMP and goes back to it"""

    def __init__(self, gmp, n, Ap, Ai, vals, q, bs, a_scale, b_scale):
        self.gmp, self.n, self.nrhs, self.z = gmp, n, len(bs), []
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
        self.opt = Options(3, 0, 1.0, 0, 128, 0)                                  # SLIP_TOL_SMALLEST, tol 1: the defaults
        self.xrows = [(Mpq * self.nrhs)() for _ in range(n)]                      # what SLIP_create_mpq_mat leaves: 0 / 1
        for r in self.xrows:
            for k in range(self.nrhs):
                getattr(gmp, "__gmpq_init")(C.byref(r[k]))
        self.x = (C.POINTER(Mpq) * n)(*[C.cast(r, C.POINTER(Mpq)) for r in self.xrows])

    def set(self, z, v):
        assert getattr(self.gmp, "__gmpz_init_set_str")(C.byref(z), format(int(v), "x").encode(), 16) == 0    # (no name mangling)
        self.z.append(z)

    def args(self):
        return [C.addressof(self.x), C.addressof(self.A), C.addressof(self.S), C.addressof(self.b), C.addressof(self.opt)]

    def solution(self, k):
        return [(mpz_value(self.xrows[i][k].num), mpz_value(self.xrows[i][k].den)) for i in range(self.n)]

    def close(self):
        for z in self.z:
            getattr(self.gmp, "__gmpz_clear")(C.byref(z))
        for r in self.xrows:
            for k in range(self.nrhs):
                getattr(self.gmp, "__gmpq_clear")(C.byref(r[k]))
        self.z, self.xrows = [], []


@pytest.mark.parametrize("name", ["solve_test_mat", "solve_10teams"])
def test_dropin_solve_mpq(libs, name):
    """A->scale = 1000, b->scale = 7/3: x = canonical(xnum * 3000, xden * 7), for the reference's own rationals of the first
    right-hand side and a handle's numerators over det of the second; both exported names"""
    import slip_lu_amd as sl
    gmp, shim = libs
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
    want = [placed([canonical(num[p] * 3000, den[p] * 7) for p in range(n)], q),
            placed([canonical(x[n + p] * 3000, det * 7) for p in range(n)], q)]
    pr = Problem(gmp, n, Ap, Ai, oracle_lib.bigints(Alen, Alimbs), q, bs, (1000, 1), (7, 3))
    try:
        for fn in (shim.SLIP_hip_solve_mpq, shim.SLIP_solve_mpq):
            assert fn(*pr.args()) == SLIP_OK
            for k in range(2):
                got = pr.solution(k)
                assert all(d > 0 for _, d in got)
                assert_same_fractions(got, want[k], (name, k))
    finally:
        pr.close()


def test_dropin_solve_mpq_rejects_null_arguments(libs):
    """SLIP_solve_mpq.c:51-55: any missing argument or array is SLIP_INCORRECT_INPUT"""
    gmp, shim = libs
    n, Ap, Ai, Alen, Alimbs, q, _ = solve_inputs(SOLVE_CASES["solve_test_mat"])
    pr = Problem(gmp, n, Ap, Ai, oracle_lib.bigints(Alen, Alimbs), q, rhs_pattern(oracle_lib.solve_rhs(n), 1), (1, 1), (1, 1))
    try:
        good = pr.args()
        for k in range(5):
            assert shim.SLIP_hip_solve_mpq(*[None if t == k else a for t, a in enumerate(good)]) == SLIP_INCORRECT_INPUT, k
        for obj, field in ((pr.A, "p"), (pr.A, "i"), (pr.A, "x"), (pr.S, "q"), (pr.b, "x")):
            ptr = getattr(obj, field)                                 # a view of the field itself: keep the address, not the view
            addr = C.cast(ptr, C.c_void_p).value
            setattr(obj, field, type(ptr)())
            assert shim.SLIP_hip_solve_mpq(*good) == SLIP_INCORRECT_INPUT, field
            setattr(obj, field, C.cast(addr, type(ptr)))
        assert shim.SLIP_hip_solve_mpq(*good) == SLIP_OK
    finally:
        pr.close()
