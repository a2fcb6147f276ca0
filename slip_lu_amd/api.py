"""Python face of the C ABI in include/slip_hip.h (tests, bench, smoke).

Mirrors the reference's expert sequence for the hot path
(SLIP_LU/Demo/SLIPLU.c:237-256): the column order q comes from the analysis
step (data to this module), `Factorization.run` is SLIP_LU_factorize.
All arithmetic happens in the HIP library; this file only marshals arrays.
"""
import ctypes as C
import os

import numpy as np

from . import _lib

STATUS = {0: "SLIP_OK", -1: "SLIP_OUT_OF_MEMORY", -2: "SLIP_SINGULAR",
          -3: "SLIP_INCORRECT_INPUT", -4: "SLIP_INCORRECT", -100: "DEVICE_ERROR"}


class SlipError(RuntimeError):
    def __init__(self, code, where):
        super().__init__(f"{where}: {STATUS.get(code, code)}")
        self.code = code


def ints_to_slab(values):
    """int64 numpy array -> (signed limb counts, limbs): |v| < 2^63."""
    v = np.asarray(values, dtype=np.int64)
    lens = np.sign(v).astype(np.int32)
    limbs = np.abs(v[v != 0]).astype(np.uint64)
    return lens, limbs


def _limb_arrays(lens, limbs):
    """(signed limb counts, limbs) as contiguous int32 / uint64 arrays, the limbs never empty (a valid pointer), and the
    capacity the C side is told: the limbs really given"""
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    limbs = np.ascontiguousarray(limbs, dtype=np.uint64)
    cap = limbs.size
    return lens, (limbs if cap else np.zeros(1, np.uint64)), cap


def _check_given_columns(K, Lp, Li, Llen, Llimbs, Up, Ui, Ulen, Ulimbs, rows, where):
    """K > 0 given columns in the form `download()` returns, `rows` K pivot rows (or pinv): the C ABI takes no capacities,
    so arrays shorter than K columns, the column pointers or the limb counts promise are refused here"""
    if Lp.size < K + 1 or Up.size < K + 1 or rows.size < K:
        raise SlipError(-3, f"{where}: arrays shorter than K columns")
    for p, idx, lens, limbs in ((Lp, Li, Llen, Llimbs), (Up, Ui, Ulen, Ulimbs)):
        nz = int(p[K])
        if nz > 0 and (idx.size < nz or lens.size < nz or int(np.abs(lens[:nz].astype(np.int64)).sum()) > limbs.size):
            raise SlipError(-3, f"{where}: arrays shorter than the column pointers or limb counts say")


def _check_result(rc, where, first, bad):
    """SLIP_INCORRECT is a verdict, every other nonzero code an error"""
    if rc not in (0, -4):
        raise SlipError(rc, where)
    return rc == 0, first, bad


def check_solution(n, Ap, Ai, Alen, Alimbs, blen, blimbs, xlen, xlimbs, dlen, dlimbs, nrhs=1, lib_path=None):
    """Exact check on the device (slip_hip_check_solution): A * x_c == d_c * b_c for every right-hand side c, with A as
    Factorization() takes it, b by original row and x by ORIGINAL column (n entries per right-hand side), d one nonzero
    denominator per right-hand side, all as limb slabs.  Returns (ok, first_bad_row int32[nrhs], bad_rows int64[nrhs])."""
    lib = _lib.load(lib_path)
    n, nrhs = int(n), int(nrhs)
    Ap = np.ascontiguousarray(Ap, dtype=np.int64)
    Ai = np.ascontiguousarray(Ai, dtype=np.int32)
    Alen, Alimbs, _ = _limb_arrays(Alen, Alimbs)
    blen, blimbs, bcap = _limb_arrays(blen, blimbs)
    xlen, xlimbs, xcap = _limb_arrays(xlen, xlimbs)
    dlen, dlimbs, dcap = _limb_arrays(dlen, dlimbs)
    if Ap.size != n + 1 or blen.size != n * nrhs or xlen.size != n * nrhs or dlen.size != nrhs:
        raise ValueError("check_solution: Ap needs n+1 entries, blen and xlen n*nrhs, dlen nrhs")
    if Ai.size == 0:
        Ai = np.zeros(1, np.int32)
    first = np.zeros(max(nrhs, 1), np.int32)
    bad = np.zeros(max(nrhs, 1), np.int64)
    rc = lib.slip_hip_check_solution(n, Ap.ctypes.data, Ai.ctypes.data, Alen.ctypes.data, Alimbs.ctypes.data, nrhs,
                                     blen.ctypes.data, blimbs.ctypes.data, bcap, xlen.ctypes.data, xlimbs.ctypes.data, xcap,
                                     dlen.ctypes.data, dlimbs.ctypes.data, dcap, first.ctypes.data, bad.ctypes.data, None)
    return _check_result(rc, "slip_hip_check_solution", first[:nrhs], bad[:nrhs])


def _int_limbs(v):
    """a Python int -> (signed limb count, limbs)"""
    a, limbs = abs(int(v)), []
    while a:
        limbs.append(a & (2 ** 64 - 1)); a >>= 64
    return (-len(limbs) if v < 0 else len(limbs)), np.array(limbs if limbs else [0], np.uint64)


def _rhs(n, blen, blimbs, nrhs):
    """the right-hand sides of a solve-and-convert as contiguous arrays (the limbs never empty) and nrhs as an int"""
    blen = np.ascontiguousarray(blen, dtype=np.int32)
    blimbs = np.ascontiguousarray(blimbs, dtype=np.uint64)
    nrhs = int(nrhs)
    if nrhs >= 1 and blen.size != n * nrhs:
        raise ValueError("blen must hold n*nrhs entries")
    return blen, (blimbs if blimbs.size else np.zeros(1, dtype=np.uint64)), nrhs


def _scale_args(scale):
    """a scale -- None, a pair (num, den) of Python ints or a Fraction -- as the four arguments of the C ABI: each part's
    signed limb count and a pointer to its limbs (None: the part is 1; the pointer keeps its array alive)"""
    if scale is None:
        return 0, None, 0, None
    num, den = (scale.numerator, scale.denominator) if hasattr(scale, "numerator") else scale
    (snlen, sn), (sdlen, sd) = _int_limbs(num), _int_limbs(den)
    return snlen, sn.ctypes.data_as(C.c_void_p), sdlen, sd.ctypes.data_as(C.c_void_p)


def _quot_args(n, nrhs, xlen, xlimbs, dlen, dlimbs, where):
    """n, nrhs and the leading arguments of slip_hip_solution_to_*: n, nrhs and the two slabs with the capacities they really
    have (the pointers keep their arrays alive)"""
    n, nrhs = int(n), int(nrhs)
    xlen, xlimbs, xcap = _limb_arrays(xlen, xlimbs)
    dlen, dlimbs, dcap = _limb_arrays(dlen, dlimbs)
    if nrhs >= 1 and (xlen.size != n * nrhs or dlen.size != nrhs):
        raise ValueError(f"{where}: xlen needs n*nrhs entries, dlen nrhs")
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    return n, nrhs, (n, nrhs, ptr(xlen), ptr(xlimbs), xcap, ptr(dlen), ptr(dlimbs), dcap)


def _paths(fn, *args):
    """the four path counters a *_paths entry point fills"""
    out = np.zeros(4, np.int64)
    fn(*args, out.ctypes.data)
    return [int(v) for v in out]


def solution_to_double(n, xlen, xlimbs, dlen, dlimbs, nrhs=1, lib_path=None):
    """Numerators over one nonzero denominator per right-hand side -> float64[nrhs, n] on the device
    (slip_hip_solution_to_double): every entry is the exact rational truncated toward zero onto the double grid, bit for bit
    what mpq_get_d returns.  x as limb slabs (n entries per right-hand side), output in the order of the input."""
    lib = _lib.load(lib_path)
    n, nrhs, args = _quot_args(n, nrhs, xlen, xlimbs, dlen, dlimbs, "solution_to_double")
    out = np.zeros((max(nrhs, 1), max(n, 1)), np.float64)
    rc = lib.slip_hip_solution_to_double(*args, out.ctypes.data, None)
    if rc:
        raise SlipError(rc, "slip_hip_solution_to_double")
    return out[:nrhs, :n]


def _take_slab(lib, pl, px, nl, count):
    """a (counts, limbs) result the library allocated -> numpy copies; the library's arrays are released"""
    lens = np.ctypeslib.as_array(C.cast(pl, C.POINTER(C.c_int32)), shape=(count,)).copy()
    limbs = (np.ctypeslib.as_array(C.cast(px, C.POINTER(C.c_uint64)), shape=(nl.value,)).copy()
             if nl.value else np.zeros(0, np.uint64))
    lib.slip_hip_free(pl)
    lib.slip_hip_free(px)
    return lens, limbs


def solution_to_rational(n, xlen, xlimbs, dlen, dlimbs, nrhs=1, lib_path=None):
    """Numerators over one nonzero denominator per right-hand side -> every entry in lowest terms on the device
    (slip_hip_solution_to_rational): (numlen, numlimbs, denlen, denlimbs), two compact limb slabs of n * nrhs entries in the
    order of the input, GMP's canonical form -- den > 0, the sign on num, 0 as 0 / 1."""
    lib = _lib.load(lib_path)
    n, nrhs, args = _quot_args(n, nrhs, xlen, xlimbs, dlen, dlimbs, "solution_to_rational")
    pnl, pnx, nnl, pdl, pdx, dnl = C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_void_p(), C.c_int64()
    rc = lib.slip_hip_solution_to_rational(*args, C.byref(pnl), C.byref(pnx), C.byref(nnl), C.byref(pdl), C.byref(pdx), C.byref(dnl),
                                           None)
    if rc:
        raise SlipError(rc, "slip_hip_solution_to_rational")
    return _take_slab(lib, pnl, pnx, nnl, n * nrhs) + _take_slab(lib, pdl, pdx, dnl, n * nrhs)


def solution_to_rational_paths(lib_path=None):
    """entries of this thread's last solution_to_rational by the path that settled them, as Factorization.to_rational_paths"""
    return _paths(_lib.load(lib_path).slip_hip_solution_to_rational_paths)


def _mpfr_outputs(count, prec):
    """the four arrays a conversion to multi-precision floats fills: sign, exp, mant[count, ceil(prec / 64)], ternary"""
    nl = (max(int(prec), 1) + 63) // 64 if int(prec) <= 65536 else 1      # a refused prec allocates nothing large
    return (np.zeros(max(count, 1), np.int8), np.zeros(max(count, 1), np.int64), np.zeros((max(count, 1), nl), np.uint64),
            np.zeros(max(count, 1), np.int8))


def solution_to_mpfr(n, xlen, xlimbs, dlen, dlimbs, nrhs=1, prec=128, rnd=0, lib_path=None):
    """Numerators over one nonzero denominator per right-hand side -> correctly rounded floats of `prec` bits on the device
    (slip_hip_solution_to_mpfr): (sign, exp, mant, ternary) of n * nrhs entries in the order of the input, every entry what
    mpfr_set_q leaves under the rounding mode rnd (MPFR_RNDN 0, RNDZ 1, RNDU 2, RNDD 3, RNDA 4): sign 0 / +1 / -1, MPFR's
    exponent, the mantissa left-aligned in ceil(prec / 64) limbs (mant[t, -1] is the top limb), the ternary value."""
    lib = _lib.load(lib_path)
    n, nrhs, args = _quot_args(n, nrhs, xlen, xlimbs, dlen, dlimbs, "solution_to_mpfr")
    count = max(n, 0) * max(nrhs, 0)
    sign, exp, mant, tern = _mpfr_outputs(count, prec)
    rc = lib.slip_hip_solution_to_mpfr(*args, int(prec), int(rnd), sign.ctypes.data, exp.ctypes.data, mant.ctypes.data,
                                       tern.ctypes.data, None)
    if rc:
        raise SlipError(rc, "slip_hip_solution_to_mpfr")
    return sign[:count], exp[:count], mant[:count], tern[:count]


def solution_to_mpfr_paths(lib_path=None):
    """entries of this thread's last solution_to_mpfr by the path that settled them, as Factorization.to_mpfr_paths"""
    return _paths(_lib.load(lib_path).slip_hip_solution_to_mpfr_paths)


def _multiply(lib, fn, handle, nx, nout, xlen, xlimbs, nvec, transpose, b, d, stream):
    """one call of slip_hip_factor_multiply / slip_hip_matrix_multiply: x holds nx entries per vector, b and the result nout;
    b and d are None or (signed limb counts, limbs)"""
    nvec = int(nvec)
    xlen, xlimbs, xcap = _limb_arrays(xlen, xlimbs)
    if nvec >= 1 and xlen.size != nx * nvec:
        raise ValueError(f"{fn}: xlen must hold {nx} entries per vector")
    args = [xlen.ctypes.data, xlimbs.ctypes.data, xcap]
    keep = []
    for name, part, count in (("b", b, nout * nvec), ("d", d, nvec)):
        if part is None:
            args += [None, None, 0]
            continue
        plen, plimbs, pcap = _limb_arrays(*part)
        if nvec >= 1 and plen.size != count:
            raise ValueError(f"{fn}: {name} must hold {count} entries")
        keep.append((plen, plimbs))
        args += [plen.ctypes.data, plimbs.ctypes.data, pcap]
    pl, px, nl = C.c_void_p(), C.c_void_p(), C.c_int64()
    rc = getattr(lib, fn)(handle, int(bool(transpose)), nvec, *args, C.byref(pl), C.byref(px), C.byref(nl), C.c_void_p(stream or 0))
    if rc:
        raise SlipError(rc, fn)
    return _take_slab(lib, pl, px, nl, nout * nvec)


def multiply_passes(lib_path=None):
    """device ms of this thread's last product (Factorization.multiply, SparseMatrix.multiply) by pass: [the widths, the offset
    scans, the products, the packing]"""
    out = np.zeros(4, np.float64)
    _lib.load(lib_path).slip_hip_multiply_passes(out.ctypes.data)
    return [float(v) for v in out]


def _ratio_key(n, key):
    """the optional tie-break keys of a ratio test as an int32 array of n entries (None stays None)"""
    if key is None:
        return None
    key = np.ascontiguousarray(key, dtype=np.int32)
    if key.size != n:
        raise ValueError("ratio_test: key must hold n entries")
    return key


def ratio_test(n, xlen, xlimbs, alen=None, alimbs=None, nprob=1, sense=1, key=None, lib_path=None):
    """The exact ratio test on the device (slip_hip_ratio_test): per problem the eligible entry (sense * a_i > 0) with the
    smallest x_i / (sense * a_i), among exact ties the smallest (key[i], i).  x and a as limb slabs of nprob * n entries;
    without a every entry is eligible and the ratio is sense * x_i (argmin / argmax of an integer vector).  Returns
    (best, nties, neligible), int32[nprob] each: best -1 and nties 0 when nothing is eligible."""
    lib = _lib.load(lib_path)
    n, nprob = int(n), int(nprob)
    xlen, xlimbs, xcap = _limb_arrays(xlen, xlimbs)
    if n >= 1 and nprob >= 1 and xlen.size != n * nprob:
        raise ValueError("ratio_test: xlen must hold n*nprob entries")
    args = [xlen.ctypes.data, xlimbs.ctypes.data, xcap]
    if alen is None and alimbs is None:
        args += [None, None, 0]
    else:
        alen, alimbs, acap = _limb_arrays(alen, alimbs)
        if n >= 1 and nprob >= 1 and alen.size != n * nprob:
            raise ValueError("ratio_test: alen must hold n*nprob entries")
        args += [alen.ctypes.data, alimbs.ctypes.data, acap]
    key = _ratio_key(n, key) if n >= 1 else None
    best, nties, nelig = (np.zeros(max(nprob, 1), np.int32) for _ in range(3))
    rc = lib.slip_hip_ratio_test(n, nprob, *args, int(sense), None if key is None else key.ctypes.data,
                                 best.ctypes.data, nties.ctypes.data, nelig.ctypes.data, None)
    if rc:
        raise SlipError(rc, "slip_hip_ratio_test")
    return best[:nprob], nties[:nprob], nelig[:nprob]


def ratio_test_paths(lib_path=None):
    """this thread's last ratio_test: [eligible entries, entries the bound pass left to the exact pass, exact comparisons that
    formed products, of those the comparisons on the memory path]"""
    return _paths(_lib.load(lib_path).slip_hip_ratio_test_paths)


class Bounds:
    """A set of bounds l_i = lo_i / den <= x_i <= hi_i / den for the bounded selections (slip_hip_bounds): kind[i] bit 0 = a
    finite lower bound, bit 1 = a finite upper bound; lo and hi are (signed limb counts, limbs) slabs of n entries (the entry of
    a side kind switches off is ignored; a side nothing switches on may be None); den a positive Python int."""

    def __init__(self, n, kind, lo=None, hi=None, den=1):
        self.n = int(n)
        self.kind = np.ascontiguousarray(kind, dtype=np.int32)
        if self.kind.size != self.n:
            raise ValueError("Bounds: kind must hold n entries")
        self.lo = None if lo is None else _limb_arrays(*lo)
        self.hi = None if hi is None else _limb_arrays(*hi)
        for s in (self.lo, self.hi):
            if s is not None and s[0].size != self.n:
                raise ValueError("Bounds: lo and hi must hold n entries")
        self.bdlen, self.bd = _int_limbs(den)
        self.rec = _lib.BoundsRec()
        self.rec.kind = self.kind.ctypes.data
        if self.lo is not None:
            self.rec.lolen, self.rec.lolimbs, self.rec.lo_limbs = self.lo[0].ctypes.data, self.lo[1].ctypes.data, self.lo[2]
        if self.hi is not None:
            self.rec.hilen, self.rec.hilimbs, self.rec.hi_limbs = self.hi[0].ctypes.data, self.hi[1].ctypes.data, self.hi[2]
        if den != 1:
            self.rec.bdlen, self.rec.bdlimbs = self.bdlen, self.bd.ctypes.data

    def ref(self, n):
        if self.n != n:
            raise ValueError("Bounds: made for another n")
        return C.byref(self.rec)


def _bounded_results(lib, rc, where, res, nprob, winners, per, pl, px, nl):
    if rc:
        raise SlipError(rc, where)
    res = tuple(r[:nprob] for r in res)
    return res + _take_slab(lib, pl, px, nl, per * nprob) if winners else res


def _bounded_slabs(mode, n, nprob, slabs, bounds, sense, key, winners, lib_path):
    lib = _lib.load(lib_path)
    n, nprob = int(n), int(nprob)
    args, keep = [], []
    for t, (lens, limbs) in enumerate(slabs):
        lens, limbs, cap = _limb_arrays(lens, limbs)
        if n >= 1 and nprob >= 1 and lens.size != (nprob if t == len(slabs) - 1 else n * nprob):
            raise ValueError("bounded selection: x and a must hold n*nprob entries, d nprob")
        keep.append((lens, limbs))
        args += [lens.ctypes.data, limbs.ctypes.data, cap]
    key = _ratio_key(n, key) if n >= 1 else None
    res = [np.zeros(max(nprob, 1), np.int32) for _ in range(4)]
    pl, px, nl = C.c_void_p(), C.c_void_p(), C.c_int64()
    outs = (C.byref(pl), C.byref(px), C.byref(nl)) if winners else (None, None, None)
    tail = [None if key is None else key.ctypes.data] + [r.ctypes.data for r in res] + list(outs) + [None]
    if mode == 0:
        rc = lib.slip_hip_ratio_test_bounded(n, nprob, *args, bounds.ref(n), int(sense), *tail)
    else:
        rc = lib.slip_hip_bound_test(n, nprob, *args, bounds.ref(n), *tail)
    return _bounded_results(lib, rc, "slip_hip_bound_test" if mode else "slip_hip_ratio_test_bounded", res, nprob, winners,
                            1 if mode else 2, pl, px, nl)


def ratio_test_bounded(n, xlen, xlimbs, alen, alimbs, dlen, dlimbs, bounds, nprob=1, sense=1, key=None, winners=False, lib_path=None):
    """The bounded ratio test on caller slabs (slip_hip_ratio_test_bounded): x and a hold nprob * n numerators over one nonzero
    signed d per problem.  With t_i = sense * sign(d) * a_i an entry heads for its lower bound (t_i > 0, bit 0 of kind, N_i =
    den * x_i - d * lo_i, a'_i = a_i, side -1) or its upper bound (t_i < 0, bit 1, N_i = d * hi_i - den * x_i, a'_i = -a_i, side
    +1); the smallest N_i / (sense * a'_i) wins, exact ties to the smallest (key[i], i).  Returns (best, nties, neligible,
    side), int32[nprob] each, with winners=True also (wlen, wlimbs): N_best and a'_best as entries 2c and 2c + 1."""
    return _bounded_slabs(0, n, nprob, ((xlen, xlimbs), (alen, alimbs), (dlen, dlimbs)), bounds, sense, key, winners, lib_path)


def bound_test(n, xlen, xlimbs, dlen, dlimbs, bounds, nprob=1, key=None, winners=False, lib_path=None):
    """The exact feasibility test on caller slabs (slip_hip_bound_test): per problem the entry that violates a bound the most
    (v_i = max(s * (d * lo_i - den * x_i), s * (den * x_i - d * hi_i)) > 0, s = sign(d)), ties to the smallest (key[i], i).
    Returns (worst, nties, nviolated, side), worst -1 when the vector is feasible; with winners=True also (wlen, wlimbs), entry
    c the violation v_worst of problem c."""
    return _bounded_slabs(1, n, nprob, ((xlen, xlimbs), (dlen, dlimbs)), bounds, 1, key, winners, lib_path)


def bound_paths(lib_path=None):
    """this thread's last handle-less bounded call: entries formed [without a product, in a lane, by a wavefront in registers,
    by a wavefront through memory], then the four counts of ratio_test_paths for its selection"""
    out = np.zeros(8, np.int64)
    _lib.load(lib_path).slip_hip_bound_paths(out.ctypes.data)
    return [int(v) for v in out]


def _scalar_slab(v, nprob, what):
    """one scalar per problem -- a (signed limb counts, limbs) slab (any pair of two arrays), a Python int or a sequence of nprob Python ints (small
    ones go through ints_to_slab, wider ones limb by limb) -- as contiguous arrays and the capacity they really have"""
    if isinstance(v, (tuple, list)) and len(v) == 2 and hasattr(v[0], "__len__") and hasattr(v[1], "__len__"):
        lens, limbs = v
    else:
        vals = [int(v)] * max(nprob, 1) if not hasattr(v, "__len__") else [int(t) for t in v]
        if all(abs(t) < 2 ** 63 for t in vals):
            lens, limbs = ints_to_slab(vals)
        else:
            parts = [_int_limbs(t) for t in vals]
            lens = np.array([l for l, _ in parts], np.int32)
            limbs = np.concatenate([x[:abs(l)] for l, x in parts]) if parts else np.zeros(0, np.uint64)
    lens, limbs, cap = _limb_arrays(lens, limbs)
    if nprob >= 1 and lens.size != nprob:
        raise ValueError(f"pivot update: {what} must hold one entry per problem")
    return lens, limbs, cap


def _place_array(place, nprob):
    if place is None:
        return None
    place = np.ascontiguousarray(place, dtype=np.int32)
    if nprob >= 1 and place.size != nprob:
        raise ValueError("pivot update: place must hold one index per problem")
    return place


def pivot_update(n, vlen, vlimbs, alen, alimbs, p, t, d=None, place=None, nprob=1, lib_path=None):
    """The exact pivot update on caller slabs (slip_hip_pivot_update): R_i = (P_c * V_i - T_c * A_i) / D_c for the nprob * n
    numerators v and a, one P, T and (optionally) one nonzero D per problem (Python ints or slabs); without d nothing is
    divided.  place: per problem an index in [-1, n) whose entry of the result is T_c itself.  Returns (rlen, rlimbs,
    ninexact): the result as a normalised slab; an entry its D does not divide has length 0 and counts in ninexact[c]."""
    lib = _lib.load(lib_path)
    n, nprob = int(n), int(nprob)
    vlen, vlimbs, vcap = _limb_arrays(vlen, vlimbs)
    alen, alimbs, acap = _limb_arrays(alen, alimbs)
    if n >= 1 and nprob >= 1 and (vlen.size != n * nprob or alen.size != n * nprob):
        raise ValueError("pivot_update: vlen and alen must hold n*nprob entries")
    pl_, pv, pcap = _scalar_slab(p, nprob, "p")
    tl_, tv, tcap = _scalar_slab(t, nprob, "t")
    args = [vlen.ctypes.data, vlimbs.ctypes.data, vcap, alen.ctypes.data, alimbs.ctypes.data, acap,
            pl_.ctypes.data, pv.ctypes.data, pcap, tl_.ctypes.data, tv.ctypes.data, tcap]
    if d is None:
        args += [None, None, 0]
    else:
        dl_, dv, dcap = _scalar_slab(d, nprob, "d")
        args += [dl_.ctypes.data, dv.ctypes.data, dcap]
    place = _place_array(place, nprob)
    nin = np.zeros(max(nprob, 1), np.int32)
    pl, px, nl = C.c_void_p(), C.c_void_p(), C.c_int64()
    rc = lib.slip_hip_pivot_update(n, nprob, *args, None if place is None else place.ctypes.data, nin.ctypes.data,
                                   C.byref(pl), C.byref(px), C.byref(nl), None)
    if rc:
        raise SlipError(rc, "slip_hip_pivot_update")
    return _take_slab(lib, pl, px, nl, n * nprob) + (nin[:nprob],)


def pivot_update_paths(lib_path=None):
    """this thread's last pivot_update: entries [that needed no arithmetic, formed in a lane, by a wavefront in registers, by a
    wavefront through memory], the inexact entries, three reserved zeros"""
    out = np.zeros(8, np.int64)
    _lib.load(lib_path).slip_hip_pivot_update_paths(out.ctypes.data)
    return [int(v) for v in out]


class StepResult:
    """What Factorization.step returns: best, nties, neligible, ninexact (int32[nprob] each), x = (rlen, rlimbs) the new
    numerators (nprob * n entries) and d = (dlen, dlimbs) the new denominators (nprob entries)."""

    def __init__(self, best, nties, neligible, ninexact, x, d):
        self.best, self.nties, self.neligible, self.ninexact, self.x, self.d = best, nties, neligible, ninexact, x, d


class Entering:
    """The entering variables of a bounded step (slip_hip_entering), one per problem, over the bounds' denominator: finite[c]
    = 1 switches on a finite range er_c / den >= 0, the distance to the variable's opposite bound; value is its current value
    ev_c / den (None: 0).  er and value are Python ints (one, or one per problem) or (signed limb counts, limbs) slabs."""

    def __init__(self, nprob, finite=None, er=None, value=None):
        self.nprob = int(nprob)
        self.rec = _lib.EnteringRec()
        self.finite = None if finite is None else np.ascontiguousarray(finite, dtype=np.int32)
        if self.finite is not None:
            if self.finite.size != self.nprob:
                raise ValueError("Entering: finite must hold one flag per problem")
            self.rec.finite = self.finite.ctypes.data
        self.er = None if er is None else _scalar_slab(er, self.nprob, "er")
        self.ev = None if value is None else _scalar_slab(value, self.nprob, "value")
        if self.er is not None:
            self.rec.erlen, self.rec.erlimbs, self.rec.er_limbs = self.er[0].ctypes.data, self.er[1].ctypes.data, self.er[2]
        if self.ev is not None:
            self.rec.evlen, self.rec.evlimbs, self.rec.ev_limbs = self.ev[0].ctypes.data, self.ev[1].ctypes.data, self.ev[2]

    def ref(self, nprob):
        if self.nprob != nprob:
            raise ValueError("Entering: made for another nprob")
        return C.byref(self.rec)


class BoundedStepResult:
    """What step_bounded returns: best, nties, neligible, side, move (0 unbounded, 1 pivot, 2 flip), ninexact (int32[nprob]
    each), x = (rlen, rlimbs) the new numerators (nprob * n entries), d = (dlen, dlimbs) the new denominators and e = (elen,
    elimbs) the entering variables' new numerators (nprob entries each)."""

    def __init__(self, best, nties, neligible, side, move, ninexact, x, d, e):
        self.best, self.nties, self.neligible, self.side, self.move, self.ninexact = best, nties, neligible, side, move, ninexact
        self.x, self.d, self.e = x, d, e


def _step_bounded_call(lib, fn, where, head, n, nprob, bounds, entering, sense, key, stream):
    res = [np.zeros(max(nprob, 1), np.int32) for _ in range(6)]
    outs = [(C.c_void_p(), C.c_void_p(), C.c_int64()) for _ in range(3)]
    rc = fn(*head, bounds.ref(n), None if entering is None else entering.ref(nprob), int(sense),
            None if key is None else key.ctypes.data, *[r.ctypes.data for r in res],
            *[C.byref(v) for o in outs for v in o], C.c_void_p(stream or 0))
    if rc:
        raise SlipError(rc, where)
    x, d, e = (_take_slab(lib, *o, cnt) for o, cnt in zip(outs, (n * nprob, nprob, nprob)))
    return BoundedStepResult(*(r[:nprob] for r in res), x, d, e)


def step_bounded(n, xlen, xlimbs, alen, alimbs, dlen, dlimbs, bounds, entering=None, nprob=1, sense=1, key=None, lib_path=None):
    """One bounded exact simplex step on caller slabs (slip_hip_step_bounded): the selection of `ratio_test_bounded`, the
    comparison of the winning step with the entering variable's own range (`Entering`), then the new numerators of a pivot
    (move 1: R_i = (den * a'_r * x_i - N_r * a_i) / d, entry best the entering variable's E = ev * a'_r + N_r, over den *
    a'_r) or of a bound flip (move 2: R_i = den * x_i - sense * er * a_i over den * d, E = (ev + sense * er) * d; an exact tie
    flips); move 0 leaves the problem's outputs empty.  Returns a BoundedStepResult."""
    lib = _lib.load(lib_path)
    n, nprob = int(n), int(nprob)
    args, keep = [], []
    for t, (lens, limbs) in enumerate(((xlen, xlimbs), (alen, alimbs), (dlen, dlimbs))):
        lens, limbs, cap = _limb_arrays(lens, limbs)
        if n >= 1 and nprob >= 1 and lens.size != (nprob if t == 2 else n * nprob):
            raise ValueError("step_bounded: x and a must hold n*nprob entries, d nprob")
        keep.append((lens, limbs))
        args += [lens.ctypes.data, limbs.ctypes.data, cap]
    key = _ratio_key(n, key) if n >= 1 else None
    return _step_bounded_call(lib, lib.slip_hip_step_bounded, "slip_hip_step_bounded", [n, nprob] + args, n, nprob, bounds, entering,
                              sense, key, None)


def step_bounded_paths(lib_path=None):
    """this thread's last handle-less step_bounded: the eight counts of `bound_paths`, the first five of `pivot_update_paths`,
    the problems [unbounded, pivoted, flipped], the scalars formed [without arithmetic, in a lane, in registers, through memory]"""
    out = np.zeros(20, np.int64)
    _lib.load(lib_path).slip_hip_step_bounded_paths(out.ctypes.data)
    return [int(v) for v in out]


def step_bounded_ms(lib_path=None):
    """device ms of this thread's last handle-less step_bounded: [the selection's form passes, the selection, the scalars, the update]"""
    out = np.zeros(4, np.float64)
    _lib.load(lib_path).slip_hip_step_bounded_ms(out.ctypes.data)
    return [float(v) for v in out]


def _states_args(ncols, state, weights, where):
    """the states and optional weights of a pricing with states as the arguments of the C ABI (and the arrays behind them)"""
    state = np.ascontiguousarray(state, dtype=np.int32)
    if state.size != ncols:
        raise ValueError(f"{where}: state must hold ncols entries")
    if weights is None:
        return (state,), [state.ctypes.data, None, None, 0]
    wlen, wlimbs, wcap = _limb_arrays(*weights)
    if wlen.size != ncols:
        raise ValueError(f"{where}: weights must hold ncols entries")
    return (state, wlen, wlimbs), [state.ctypes.data, wlen.ctypes.data, wlimbs.ctypes.data, wcap]


def price_select(ncols, xlen, xlimbs, dlen, dlimbs, state, alen=None, alimbs=None, weights=None, nprob=1, sides=1, sense=1,
                 key=None, winners=False, lib_path=None):
    """Pricing with nonbasic states on caller slabs (slip_hip_price_select): x (and a, iff sides=2) hold nprob * ncols
    numerators X_j (A_j) over one nonzero signed d per problem; state[j] is 0 (never eligible), 1 (at lower), 2 (at upper) or
    3 (free); weights is None or a (signed limb counts, limbs) slab of ncols positive integers (sides=1 only).  With v_j =
    X_j / d: sides=1 picks the eligible j (sense * v_j < 0 at lower, > 0 at upper, v_j != 0 free) with the largest |v_j|, or
    v_j^2 / w_j with weights; sides=2 the eligible j (t_j = sense * sign(d) * A_j > 0 at lower, < 0 at upper, != 0 free) with
    the smallest X_j / (sense * A_j).  Exact ties go to the smallest (key[j], j).  Returns (best, nties, neligible, vsign),
    int32[nprob] each, vsign the sign of v_best; with winners=True also (wlen, wlimbs): X_best and A_best of problem c as
    entries 2c and 2c + 1 (sides=1: the second one empty), both empty where best is -1."""
    lib = _lib.load(lib_path)
    ncols, nprob, sides = int(ncols), int(nprob), int(sides)
    xlen, xlimbs, xcap = _limb_arrays(xlen, xlimbs)
    dlen, dlimbs, dcap = _limb_arrays(dlen, dlimbs)
    if ncols >= 1 and nprob >= 1 and (xlen.size != ncols * nprob or dlen.size != nprob):
        raise ValueError("price_select: x must hold ncols*nprob entries, d nprob")
    args = [xlen.ctypes.data, xlimbs.ctypes.data, xcap]
    if alen is None and alimbs is None:
        args += [None, None, 0]
    else:
        alen, alimbs, acap = _limb_arrays(alen, alimbs)
        if ncols >= 1 and nprob >= 1 and alen.size != ncols * nprob:
            raise ValueError("price_select: a must hold ncols*nprob entries")
        args += [alen.ctypes.data, alimbs.ctypes.data, acap]
    args += [dlen.ctypes.data, dlimbs.ctypes.data, dcap]
    keep, sargs = _states_args(max(ncols, 0), state, weights, "price_select")
    key = _ratio_key(ncols, key) if ncols >= 1 else None
    res = [np.zeros(max(nprob, 1), np.int32) for _ in range(4)]
    pl, px, nl = C.c_void_p(), C.c_void_p(), C.c_int64()
    outs = (C.byref(pl), C.byref(px), C.byref(nl)) if winners else (None, None, None)
    rc = lib.slip_hip_price_select(ncols, nprob, sides, *args, *sargs, int(sense), None if key is None else key.ctypes.data,
                                   *[r.ctypes.data for r in res], *outs, None)
    return _bounded_results(lib, rc, "slip_hip_price_select", res, nprob, winners, 2, pl, px, nl)


def price_select_paths(lib_path=None):
    """this thread's last price_select: eligible entries [settled without a product, squared in a lane, squared by a
    wavefront in registers, squared by a wavefront through memory], then the four counts of ratio_test_paths for its selection"""
    out = np.zeros(8, np.int64)
    _lib.load(lib_path).slip_hip_price_select_paths(out.ctypes.data)
    return [int(v) for v in out]


class SparseMatrix:
    """An m x ncols integer matrix resident on one GPU without a factorisation (handle of slip_hip_matrix_*): the CSC as
    Factorization() takes it, a repeated row keeping its LAST value."""

    def __init__(self, m, ncols, Ap, Ai, Alen, Alimbs, lib_path=None):
        self.lib = _lib.load(lib_path)
        self.m, self.ncols = int(m), int(ncols)
        Ap = np.ascontiguousarray(Ap, dtype=np.int64)
        Ai = np.ascontiguousarray(Ai, dtype=np.int32)
        Alen, Alimbs, _ = _limb_arrays(Alen, Alimbs)
        if self.ncols >= 0 and Ap.size != self.ncols + 1:
            raise ValueError("SparseMatrix: Ap needs ncols+1 entries")
        if Ai.size == 0:
            Ai, Alen = np.zeros(1, np.int32), np.zeros(1, np.int32)
        self.h = C.c_void_p()
        rc = self.lib.slip_hip_matrix_create(C.byref(self.h), self.m, self.ncols, Ap.ctypes.data, Ai.ctypes.data,
                                             Alen.ctypes.data, Alimbs.ctypes.data)
        if rc:
            self.h = None
            raise SlipError(rc, "slip_hip_matrix_create")

    def multiply(self, xlen, xlimbs, nvec=1, transpose=False, b=None, d=None, stream=None):
        """The exact product on the device (slip_hip_matrix_multiply): r_c = M x_c - d_c b_c (x: ncols entries per vector, r
        and b: m), with transpose=True r_c = M^T x_c - d_c b_c (x: m, r and b: ncols).  b, d: None or (signed limb counts,
        limbs), d one nonzero value per vector and required with b.  Returns (rlen, rlimbs), normalised."""
        nx, nout = (self.m, self.ncols) if transpose else (self.ncols, self.m)
        return _multiply(self.lib, "slip_hip_matrix_multiply", self.h, nx, nout, xlen, xlimbs, nvec, transpose, b, d, stream)

    def multiply_ms(self):
        """device ms of the kernels of the last multiply"""
        return self.lib.slip_hip_matrix_multiply_ms(self.h)

    def close(self):
        if getattr(self, "h", None):
            self.lib.slip_hip_matrix_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def matgen(n, density, bits, seed, lib_path=None):
    """The benchmark's synthetic CSC (slip_matgen.h) -> Ap, Ai, Ax (int64 values)."""
    lib = _lib.load(lib_path)
    pAp, pAi, pAx = C.c_void_p(), C.c_void_p(), C.c_void_p()
    rc = lib.slip_hip_matgen(n, density, bits, seed, C.byref(pAp), C.byref(pAi), C.byref(pAx))
    if rc:
        raise SlipError(rc, "slip_hip_matgen")
    Ap = np.ctypeslib.as_array(C.cast(pAp, C.POINTER(C.c_int64)), shape=(n + 1,)).copy()
    nnz = int(Ap[n])
    Ai = np.ctypeslib.as_array(C.cast(pAi, C.POINTER(C.c_int32)), shape=(nnz,)).copy()
    Ax = np.ctypeslib.as_array(C.cast(pAx, C.POINTER(C.c_int64)), shape=(nnz,)).copy()
    for p in (pAp, pAi, pAx):
        lib.slip_hip_free(p)
    return Ap, Ai, Ax


def read_triplet(path, lib_path=None):
    """A triplet file (SLIP_tripread's format, SLIP_LU/Demo/demos.c:245-331) -> n, Ap, Ai, Alen, Alimbs: the CSC limb slabs
    SLIP_build_sparse_trip_mpz would hold (slip_trip_to_mat.c:23-69), ready for Factorization()."""
    lib = _lib.load(lib_path)
    n, nl = C.c_int32(), C.c_int64()
    pAp, pAi, pAlen, pAl = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    rc = lib.slip_hip_read_triplet(os.fsencode(path), C.byref(n), C.byref(pAp), C.byref(pAi), C.byref(pAlen), C.byref(pAl), C.byref(nl))
    if rc:
        raise SlipError(rc, "slip_hip_read_triplet")
    n = n.value
    Ap = np.ctypeslib.as_array(C.cast(pAp, C.POINTER(C.c_int64)), shape=(n + 1,)).copy()
    nnz = int(Ap[n])
    Ai = np.ctypeslib.as_array(C.cast(pAi, C.POINTER(C.c_int32)), shape=(nnz,)).copy()
    Alen = np.ctypeslib.as_array(C.cast(pAlen, C.POINTER(C.c_int32)), shape=(nnz,)).copy()
    Al = np.ctypeslib.as_array(C.cast(pAl, C.POINTER(C.c_uint64)), shape=(max(nl.value, 1),)).copy()[:nl.value]
    for p in (pAp, pAi, pAlen, pAl):
        lib.slip_hip_free(p)
    return n, Ap, Ai, Alen, Al


def write_triplet(path, n, Ap, Ai, Alen, Alimbs, lib_path=None):
    """CSC limb slabs -> a triplet file (1-based, decimal) that SLIP_tripread and read_triplet accept."""
    lib = _lib.load(lib_path)
    Ap = np.ascontiguousarray(Ap, np.int64); Ai = np.ascontiguousarray(Ai, np.int32)
    Alen = np.ascontiguousarray(Alen, np.int32); Al = np.ascontiguousarray(Alimbs, np.uint64)
    if Al.size == 0:
        Al = np.zeros(1, np.uint64)
    rc = lib.slip_hip_write_triplet(os.fsencode(path), int(n), Ap.ctypes.data, Ai.ctypes.data, Alen.ctypes.data, Al.ctypes.data)
    if rc:
        raise SlipError(rc, "slip_hip_write_triplet")


class Factorization:
    """A resident REF LU factorisation on one GPU (handle of slip_hip_factor_*)."""

    def __init__(self, n, Ap, Ai, Alen, Alimbs, q, pivot=3, tol=1.0, limb_cap=0, waves=0,
                 lnz_hint=0, unz_hint=0, workers=0, lib_path=None, debug_flags=0):
        self.lib = _lib.load(lib_path)
        self.n = int(n)
        Ap = np.ascontiguousarray(Ap, dtype=np.int64)
        Ai = np.ascontiguousarray(Ai, dtype=np.int32)
        Alen = np.ascontiguousarray(Alen, dtype=np.int32)
        Alimbs = np.ascontiguousarray(Alimbs, dtype=np.uint64)
        if Alimbs.size == 0:
            Alimbs = np.zeros(1, dtype=np.uint64)
        q = np.ascontiguousarray(q, dtype=np.int32)
        opt = _lib.Options(pivot, tol, limb_cap, waves, lnz_hint, unz_hint, workers, debug_flags)
        self.h = C.c_void_p()
        rc = self.lib.slip_hip_factor_create(C.byref(self.h), self.n, Ap.ctypes.data, Ai.ctypes.data,
                                             Alen.ctypes.data, Alimbs.ctypes.data, q.ctypes.data,
                                             C.byref(opt))
        if rc:
            self.h = None
            raise SlipError(rc, "slip_hip_factor_create")

    @classmethod
    def from_factors(cls, fac, waves=0, workers=0, lib_path=None):
        """A solve-only handle around factors in the form `download()` returns (slip_hip_factor_from_factors)."""
        self = cls.__new__(cls)
        self.lib = _lib.load(lib_path)
        self.n = int(fac["n"])
        arrs = [np.ascontiguousarray(fac[k], dtype=t) for k, t in (
            ("Lp", np.int64), ("Li", np.int32), ("Llen", np.int32), ("Llimbs", np.uint64),
            ("Up", np.int64), ("Ui", np.int32), ("Ulen", np.int32), ("Ulimbs", np.uint64), ("pinv", np.int32))]
        if self.n > 0:
            _check_given_columns(self.n, *arrs, "from_factors")
        arrs = [a if a.size else np.zeros(1, a.dtype) for a in arrs]
        opt = _lib.Options(3, 1.0, 0, waves, 0, 0, workers, 0)
        self.h = C.c_void_p()
        rc = self.lib.slip_hip_factor_from_factors(C.byref(self.h), self.n, *[a.ctypes.data for a in arrs], C.byref(opt))
        if rc:
            self.h = None
            raise SlipError(rc, "slip_hip_factor_from_factors")
        return self

    def set_prefix(self, K, fac, piv_row):
        """The first K columns are given (slip_hip_factor_set_prefix): `fac` holds Lp/Li/Llen/Llimbs/Up/Ui/Ulen/Ulimbs of
        those columns in the form `download()` returns, piv_row[k] the pivot row of column k; run() continues at column K."""
        K = int(K)
        arrs = [np.ascontiguousarray(fac[k], dtype=t) for k, t in (
            ("Lp", np.int64), ("Li", np.int32), ("Llen", np.int32), ("Llimbs", np.uint64),
            ("Up", np.int64), ("Ui", np.int32), ("Ulen", np.int32), ("Ulimbs", np.uint64))]
        arrs.append(np.ascontiguousarray(piv_row, dtype=np.int32))
        if K > 0:
            _check_given_columns(K, *arrs, "set_prefix")
        arrs = [a if a.size else np.zeros(1, a.dtype) for a in arrs]
        rc = self.lib.slip_hip_factor_set_prefix(self.h, K, *[a.ctypes.data for a in arrs])
        if rc:
            raise SlipError(rc, "slip_hip_factor_set_prefix")

    def reset(self):
        rc = self.lib.slip_hip_factor_reset(self.h)
        if rc:
            raise SlipError(rc, "slip_hip_factor_reset")

    def rewind(self, K, q_tail=None, stream=None):
        """Back to column K (slip_hip_factor_rewind): the state run(K) from a reset would have left, 0 <= K <= info()["K"];
        run() continues with column K.  q_tail: None, or the new order of positions K..n-1 (original column ids, a
        permutation of the ids that stand there now)."""
        qt = None
        if q_tail is not None:
            qt = np.ascontiguousarray(q_tail, dtype=np.int32)
            if qt.size != self.n - int(K):
                raise SlipError(-3, "rewind: q_tail must hold n - K column ids")
            if qt.size == 0:
                qt = np.zeros(1, np.int32)
        rc = self.lib.slip_hip_factor_rewind(self.h, int(K), None if qt is None else qt.ctypes.data, C.c_void_p(stream or 0))
        if rc:
            raise SlipError(rc, "slip_hip_factor_rewind")

    def replace_column(self, j, rows, values=None, slab=None, stream=None):
        """Column j of A (original column id) gets new content on the device (slip_hip_factor_replace_column): `rows` row
        ids and `values` Python ints of any size (through ints_to_slab while they fit 63 bits), or slab=(signed limb counts,
        limbs) as Factorization() takes a column.  A repeated row keeps its LAST value.  The handle is rewound to the
        column's position if it was factorised already; run() continues from there."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        if slab is not None:
            lens, limbs = slab
        elif all(abs(int(v)) < 2 ** 63 for v in values):
            lens, limbs = ints_to_slab([int(v) for v in values])
        else:
            parts = [_int_limbs(v) for v in values]
            lens = [l for l, _ in parts]
            limbs = np.concatenate([x[:abs(l)] for l, x in parts]) if parts else np.zeros(0, np.uint64)
        lens, limbs, cap = _limb_arrays(lens, limbs)
        if lens.size != rows.size:
            raise SlipError(-3, "replace_column: one value per row id")
        if rows.size == 0:
            rows, lens = np.zeros(1, np.int32), np.zeros(1, np.int32)
            nz = 0
        else:
            nz = int(rows.size)
        rc = self.lib.slip_hip_factor_replace_column(self.h, int(j), nz, rows.ctypes.data, lens.ctypes.data, limbs.ctypes.data,
                                                     cap, C.c_void_p(stream or 0))
        if rc:
            raise SlipError(rc, "slip_hip_factor_replace_column")

    def a_storage(self):
        """the storage of the resident A: dict(nnz, nnz_cap, limbs, limbs_cap) -- live entries, entries the arrays can hold,
        live limbs, limbs the slab can hold (slip_hip_factor_a_storage)"""
        out = np.zeros(4, np.int64)
        rc = self.lib.slip_hip_factor_a_storage(self.h, out.ctypes.data)
        if rc:
            raise SlipError(rc, "slip_hip_factor_a_storage")
        return dict(nnz=int(out[0]), nnz_cap=int(out[1]), limbs=int(out[2]), limbs_cap=int(out[3]))

    def run(self, kmax=0, stream=None, check=True):
        rc = self.lib.slip_hip_factor_run(self.h, int(kmax), C.c_void_p(stream or 0))
        if rc and check:
            raise SlipError(rc, "slip_hip_factor_run")
        return rc

    def info(self):
        i = _lib.Info()
        self.lib.slip_hip_factor_info(self.h, C.byref(i))
        return {k: getattr(i, k) for k, _ in _lib.Info._fields_}

    def download(self, limb_capacity=None):
        """Factor arrays in the canonical form the tests compare (original row ids).  limb_capacity: the capacity to CLAIM for
        the L limb array (tests of the capacity check; the array itself is always sized from info())."""
        i = self.info()
        K = i["K"]
        out = dict(n=self.n, K=K, status=i["status"],
                   Lp=np.zeros(K + 1, np.int64), Up=np.zeros(K + 1, np.int64),
                   Li=np.zeros(i["lnz"], np.int32), Ui=np.zeros(i["unz"], np.int32),
                   Llen=np.zeros(i["lnz"], np.int32), Ulen=np.zeros(i["unz"], np.int32),
                   Llimbs=np.zeros(max(i["l_limbs"], 1), np.uint64), Ulimbs=np.zeros(max(i["u_limbs"], 1), np.uint64),
                   rholen=np.zeros(K, np.int32), pinv=np.zeros(self.n, np.int32))
        # pivots are entries of L: an upper bound of their limbs is l_limbs
        rho = np.zeros(max(i["l_limbs"], 1), np.uint64)
        cap = C.c_int64(rho.size)
        lcap, ucap = C.c_int64(limb_capacity if limb_capacity is not None else out["Llimbs"].size), C.c_int64(out["Ulimbs"].size)
        rc = self.lib.slip_hip_factor_download(
            self.h, out["Lp"].ctypes.data, out["Li"].ctypes.data, out["Llen"].ctypes.data, out["Llimbs"].ctypes.data, C.byref(lcap),
            out["Up"].ctypes.data, out["Ui"].ctypes.data, out["Ulen"].ctypes.data, out["Ulimbs"].ctypes.data, C.byref(ucap),
            out["rholen"].ctypes.data, rho.ctypes.data, C.byref(cap), out["pinv"].ctypes.data)
        if rc:
            raise SlipError(rc, "slip_hip_factor_download")
        out["Llimbs"] = out["Llimbs"][:lcap.value]
        out["Ulimbs"] = out["Ulimbs"][:ucap.value]
        out["rholimbs"] = rho[:cap.value].copy()
        out["counters"] = np.array([i["n_upd"], i["b_read"], i["b_write"], i["n_src"], i["l_streamed"],
                                    i["max_limbs"], K, i["limb_macs"]], dtype=np.int64)
        out["info"] = i
        return out

    def solve(self, blen, blimbs, nrhs=1, stream=None):
        """REF forward/back substitution on the resident factors (slip_hip_factor_solve): dense b in
        original row order as a limb slab -> (xlen, xlimbs) numerators over det by pivot position."""
        return self._solve("slip_hip_factor_solve", blen, blimbs, nrhs, stream)

    def solve_transpose(self, blen, blimbs, nrhs=1, stream=None):
        """The transposed system on the same resident factors (slip_hip_factor_solve_transpose): A(:,q)^T x = b, no second
        factorisation.  b is dense by pivot POSITION -- b[c*n + k] pairs with column q[k] of A -- and the numerators over
        det = rho[n-1] (the denominator of `solve`) come back by ORIGINAL row id: x[c*n + i] is for row i of A.  To solve
        A^T x = b_orig, pass b[k] = b_orig[q[k]]:

            xlen, xlimbs = f.solve_transpose(*ints_to_slab(b_orig[q]))      # x[i] = xnum[i] / det

        Returns (xlen, xlimbs) as `solve` does."""
        return self._solve("slip_hip_factor_solve_transpose", blen, blimbs, nrhs, stream)

    def _solve(self, fn, blen, blimbs, nrhs, stream):
        blen = np.ascontiguousarray(blen, dtype=np.int32)
        blimbs = np.ascontiguousarray(blimbs, dtype=np.uint64)
        if blen.size != self.n * nrhs:
            raise ValueError("blen must hold n*nrhs entries")
        if blimbs.size == 0:
            blimbs = np.zeros(1, dtype=np.uint64)
        pl, px, nl = C.c_void_p(), C.c_void_p(), C.c_int64()
        rc = getattr(self.lib, fn)(self.h, int(nrhs), blen.ctypes.data, blimbs.ctypes.data,
                                   C.byref(pl), C.byref(px), C.byref(nl), C.c_void_p(stream or 0))
        if rc:
            raise SlipError(rc, fn)
        return _take_slab(self.lib, pl, px, nl, self.n * nrhs)

    def solve_double(self, blen, blimbs, nrhs=1, transpose=False, scale=None, stream=None):
        """Solve and convert on the device (slip_hip_factor_solve_double): float64[nrhs, n], every entry the exact rational
        scale * xnum / det truncated toward zero onto the double grid (what SLIP_solve_double returns through mpq_get_d).
        Only the doubles come back.  b as `solve` takes it, the result in ORIGINAL column order (x[c, q[p]]); with
        transpose=True b as `solve_transpose` takes it, the result by original row id.  scale: a pair (num, den) of Python
        ints or a Fraction, both parts nonzero."""
        blen, blimbs, nrhs = _rhs(self.n, blen, blimbs, nrhs)
        out = np.zeros((max(nrhs, 1), self.n), np.float64)
        rc = self.lib.slip_hip_factor_solve_double(self.h, int(bool(transpose)), nrhs, blen.ctypes.data, blimbs.ctypes.data,
                                                   *_scale_args(scale), out.ctypes.data, C.c_void_p(stream or 0))
        if rc:
            raise SlipError(rc, "slip_hip_factor_solve_double")
        return out[:nrhs]

    def to_double_ms(self):
        """device ms of the conversion kernel of the last solve_double"""
        return self.lib.slip_hip_factor_to_double_ms(self.h)

    def to_double_slow(self):
        """entries of the last solve_double that the lane pass left to the exact wave pass"""
        return self.lib.slip_hip_factor_to_double_slow(self.h)

    def solve_rational(self, blen, blimbs, nrhs=1, transpose=False, scale=None, stream=None):
        """Solve and reduce on the device (slip_hip_factor_solve_rational): (numlen, numlimbs, denlen, denlimbs), entry
        c*n + j the exact rational scale * xnum / det in lowest terms, GMP's canonical form (den > 0, the sign on num, 0 as
        0 / 1: what SLIP_solve_mpq returns).  Only these two compact slabs come back.  b, transpose, scale and the order of
        the result as `solve_double`: ORIGINAL column order for the plain solve, original row id for the transposed one."""
        blen, blimbs, nrhs = _rhs(self.n, blen, blimbs, nrhs)
        pnl, pnx, nnl, pdl, pdx, dnl = C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_void_p(), C.c_int64()
        rc = self.lib.slip_hip_factor_solve_rational(self.h, int(bool(transpose)), nrhs, blen.ctypes.data, blimbs.ctypes.data,
                                                     *_scale_args(scale), C.byref(pnl), C.byref(pnx), C.byref(nnl), C.byref(pdl), C.byref(pdx), C.byref(dnl),
                                                     C.c_void_p(stream or 0))
        if rc:
            raise SlipError(rc, "slip_hip_factor_solve_rational")
        return _take_slab(self.lib, pnl, pnx, nnl, self.n * nrhs) + _take_slab(self.lib, pdl, pdx, dnl, self.n * nrhs)

    def to_rational_ms(self):
        """device ms of the reduction kernel of the last solve_rational"""
        return self.lib.slip_hip_factor_to_rational_ms(self.h)

    def to_rational_paths(self):
        """entries of the last solve_rational settled by [the lane pass, the register wave pass with g = 1, the same with
        g > 1, the memory class]"""
        return _paths(self.lib.slip_hip_factor_to_rational_paths, self.h)

    def solve_mpfr(self, blen, blimbs, nrhs=1, transpose=False, scale=None, prec=128, rnd=0, stream=None):
        """Solve and round on the device (slip_hip_factor_solve_mpfr): (sign, exp, mant, ternary), entry c*n + j the exact
        rational scale * xnum / det rounded ONCE to `prec` bits under the rounding mode rnd (MPFR_RNDN 0, RNDZ 1, RNDU 2,
        RNDD 3, RNDA 4), as mpfr_set_q leaves it (what SLIP_solve_mpfr returns): sign int8 (0 for +0), MPFR's exponent int64,
        mant uint64[nrhs*n, ceil(prec / 64)] left-aligned (mant[t, -1] is the top limb), the ternary value int8.  Only these
        come back.  b, transpose, scale and the order of the result as `solve_double`."""
        blen, blimbs, nrhs = _rhs(self.n, blen, blimbs, nrhs)
        count = self.n * max(nrhs, 0)
        sign, exp, mant, tern = _mpfr_outputs(count, prec)
        rc = self.lib.slip_hip_factor_solve_mpfr(self.h, int(bool(transpose)), nrhs, blen.ctypes.data, blimbs.ctypes.data,
                                                 *_scale_args(scale), int(prec), int(rnd), sign.ctypes.data, exp.ctypes.data, mant.ctypes.data,
                                                 tern.ctypes.data, C.c_void_p(stream or 0))
        if rc:
            raise SlipError(rc, "slip_hip_factor_solve_mpfr")
        return sign[:count], exp[:count], mant[:count], tern[:count]

    def to_mpfr_ms(self):
        """device ms of the conversion kernel of the last solve_mpfr"""
        return self.lib.slip_hip_factor_to_mpfr_ms(self.h)

    def to_mpfr_paths(self):
        """entries of the last solve_mpfr settled by [the lane pass within 64 bits, the wave pass with a denominator of at
        most 256 digits, the wave pass with a wider one, as zero]"""
        return _paths(self.lib.slip_hip_factor_to_mpfr_paths, self.h)

    def check(self, blen, blimbs, xlen, xlimbs, nrhs=1, stream=None):
        """Exact check of a solve on the device (slip_hip_factor_check): A(:,q) xnum_c == det b_c, with b as `solve` takes
        it and (xlen, xlimbs) as `solve` returns them.  Returns (ok, first_bad_row int32[nrhs], bad_rows int64[nrhs])."""
        return self._check("slip_hip_factor_check", blen, blimbs, xlen, xlimbs, nrhs, stream)

    def check_transpose(self, blen, blimbs, xlen, xlimbs, nrhs=1, stream=None):
        """Exact check of a transposed solve on the device (slip_hip_factor_check_transpose): for every position k,
        sum_i A(i, q[k]) xnum_c[i] == det b_c[k], with b as `solve_transpose` takes it (by position) and (xlen, xlimbs) as it
        returns them (by original row id).  Returns (ok, first_bad_pos int32[nrhs], bad_pos int64[nrhs])."""
        return self._check("slip_hip_factor_check_transpose", blen, blimbs, xlen, xlimbs, nrhs, stream)

    def _check(self, fn, blen, blimbs, xlen, xlimbs, nrhs, stream):
        nrhs = int(nrhs)
        blen, blimbs, bcap = _limb_arrays(blen, blimbs)
        xlen, xlimbs, xcap = _limb_arrays(xlen, xlimbs)
        if blen.size != self.n * nrhs or xlen.size != self.n * nrhs:
            raise ValueError("blen and xlen must hold n*nrhs entries")
        first = np.zeros(max(nrhs, 1), np.int32)
        bad = np.zeros(max(nrhs, 1), np.int64)
        rc = getattr(self.lib, fn)(self.h, nrhs, blen.ctypes.data, blimbs.ctypes.data, bcap,
                                   xlen.ctypes.data, xlimbs.ctypes.data, xcap, first.ctypes.data, bad.ctypes.data,
                                   C.c_void_p(stream or 0))
        return _check_result(rc, fn, first[:nrhs], bad[:nrhs])

    def check_ms(self):
        return self.lib.slip_hip_factor_check_ms(self.h)

    def multiply(self, xlen, xlimbs, nvec=1, transpose=False, b=None, d=None, stream=None):
        """The exact product with the resident A on the device (slip_hip_factor_multiply): r_c = A(:,q) x_c - d_c b_c with x
        by pivot position as `solve` returns it, r and b by original row; with transpose=True r_c = A(:,q)^T x_c - d_c b_c
        with x by original row id as `solve_transpose` returns it, r and b by position.  b, d: None or (signed limb counts,
        limbs); b alone: d = det (needs the complete factorisation); without b the product alone, in any state of the
        factorisation.  Returns (rlen, rlimbs), normalised: a zero has count 0 and no limbs."""
        return _multiply(self.lib, "slip_hip_factor_multiply", self.h, self.n, self.n, xlen, xlimbs, nvec, transpose, b, d, stream)

    def multiply_ms(self):
        """device ms of the kernels of the last multiply"""
        return self.lib.slip_hip_factor_multiply_ms(self.h)

    def ratio_test(self, blen, blimbs, nprob=1, transpose=False, sense=1, key=None, winners=False, stream=None):
        """Solve and select on the device (slip_hip_factor_ratio_test): b holds 2 * nprob right-hand sides as `solve` (or with
        transpose=True `solve_transpose`) takes them, column 2c the x side and column 2c + 1 the a side of problem c.  Per
        problem the entry with the smallest xnum_i / (sense * anum_i) among those with sense * sign(det) * anum_i > 0, exact
        ties broken by the smallest (key[i], i); indices are those of the matching solve's output (pivot position, or
        original row id when transposed).  Returns (best, nties, neligible), int32[nprob] each; with winners=True also
        (wlen, wlimbs), the slab of the winners' numerators: xnum_best and anum_best of problem c as entries 2c and 2c + 1,
        empty where best is -1.  No numerator of the solve is downloaded otherwise."""
        nprob = int(nprob)
        blen, blimbs, _ = _rhs(self.n, blen, blimbs, 2 * nprob if nprob >= 1 else nprob)
        key = _ratio_key(self.n, key)
        best, nties, nelig = (np.zeros(max(nprob, 1), np.int32) for _ in range(3))
        pl, px, nl = C.c_void_p(), C.c_void_p(), C.c_int64()
        outs = (C.byref(pl), C.byref(px), C.byref(nl)) if winners else (None, None, None)
        rc = self.lib.slip_hip_factor_ratio_test(self.h, int(bool(transpose)), nprob, blen.ctypes.data, blimbs.ctypes.data,
                                                 int(sense), None if key is None else key.ctypes.data,
                                                 best.ctypes.data, nties.ctypes.data, nelig.ctypes.data, *outs, C.c_void_p(stream or 0))
        if rc:
            raise SlipError(rc, "slip_hip_factor_ratio_test")
        res = (best[:nprob], nties[:nprob], nelig[:nprob])
        return res + _take_slab(self.lib, pl, px, nl, 2 * nprob) if winners else res

    def ratio_test_ms(self):
        """device ms of the selection kernels of the last ratio_test (the substitution: solve_ms / solve_transpose_ms)"""
        return self.lib.slip_hip_factor_ratio_test_ms(self.h)

    def ratio_test_paths(self):
        """the last ratio_test: [eligible entries, entries the bound pass left to the exact pass, exact comparisons that formed
        products, of those the comparisons on the memory path]"""
        return _paths(self.lib.slip_hip_factor_ratio_test_paths, self.h)

    def _bounded(self, mode, blen, blimbs, bounds, nprob, transpose, sense, key, winners, stream):
        nprob, per = int(nprob), 1 if mode else 2
        blen, blimbs, _ = _rhs(self.n, blen, blimbs, per * nprob if nprob >= 1 else nprob)
        key = _ratio_key(self.n, key)
        res = [np.zeros(max(nprob, 1), np.int32) for _ in range(4)]
        pl, px, nl = C.c_void_p(), C.c_void_p(), C.c_int64()
        outs = (C.byref(pl), C.byref(px), C.byref(nl)) if winners else (None, None, None)
        tail = [None if key is None else key.ctypes.data] + [r.ctypes.data for r in res] + list(outs) + [C.c_void_p(stream or 0)]
        head = (self.h, int(bool(transpose)), nprob, blen.ctypes.data, blimbs.ctypes.data, bounds.ref(self.n))
        if mode == 0:
            rc = self.lib.slip_hip_factor_ratio_test_bounded(*head, int(sense), *tail)
        else:
            rc = self.lib.slip_hip_factor_bound_test(*head, *tail)
        return _bounded_results(self.lib, rc, "slip_hip_factor_bound_test" if mode else "slip_hip_factor_ratio_test_bounded",
                                res, nprob, winners, per, pl, px, nl)

    def ratio_test_bounded(self, blen, blimbs, bounds, nprob=1, transpose=False, sense=1, key=None, winners=False, stream=None):
        """Solve and select on the device with bounds on the basic variables (slip_hip_factor_ratio_test_bounded): the
        right-hand sides and index conventions of `ratio_test`, the definition of the module's `ratio_test_bounded` with d =
        det.  Returns (best, nties, neligible, side[, wlen, wlimbs])."""
        return self._bounded(0, blen, blimbs, bounds, nprob, transpose, sense, key, winners, stream)

    def bound_test(self, blen, blimbs, bounds, nprob=1, transpose=False, key=None, winners=False, stream=None):
        """Solve and test feasibility on the device (slip_hip_factor_bound_test): nprob right-hand sides as the matching solve
        takes them, the definition of the module's `bound_test` with d = det.  Returns (worst, nties, nviolated, side[, wlen,
        wlimbs])."""
        return self._bounded(1, blen, blimbs, bounds, nprob, transpose, 1, key, winners, stream)

    def bound_ms(self):
        """device ms of the last bounded call: [the classify, offset and form passes, the selection]"""
        out = np.zeros(2, np.float64)
        self.lib.slip_hip_factor_bound_ms(self.h, out.ctypes.data)
        return [float(v) for v in out]

    def bound_paths(self):
        """the last bounded call, as the module's `bound_paths`"""
        out = np.zeros(8, np.int64)
        self.lib.slip_hip_factor_bound_paths(self.h, out.ctypes.data)
        return [int(v) for v in out]

    def solve_update(self, blen, blimbs, p, t, nprob=1, transpose=False, place=None, stream=None):
        """Solve and update on the device (slip_hip_factor_solve_update): b holds 2 * nprob right-hand sides as `ratio_test`
        takes them (2c the V side, 2c + 1 the A side); the module's `pivot_update` on the solve's numerators with D = det, P
        and T (Python ints or slabs) from the caller, indices those of the matching solve's output.  Returns (rlen, rlimbs,
        ninexact)."""
        nprob = int(nprob)
        blen, blimbs, _ = _rhs(self.n, blen, blimbs, 2 * nprob if nprob >= 1 else nprob)
        pl_, pv, pcap = _scalar_slab(p, nprob, "p")
        tl_, tv, tcap = _scalar_slab(t, nprob, "t")
        place = _place_array(place, nprob)
        nin = np.zeros(max(nprob, 1), np.int32)
        pl, px, nl = C.c_void_p(), C.c_void_p(), C.c_int64()
        rc = self.lib.slip_hip_factor_solve_update(self.h, int(bool(transpose)), nprob, blen.ctypes.data, blimbs.ctypes.data,
                                                   pl_.ctypes.data, pv.ctypes.data, pcap, tl_.ctypes.data, tv.ctypes.data, tcap,
                                                   None if place is None else place.ctypes.data, nin.ctypes.data,
                                                   C.byref(pl), C.byref(px), C.byref(nl), C.c_void_p(stream or 0))
        if rc:
            raise SlipError(rc, "slip_hip_factor_solve_update")
        return _take_slab(self.lib, pl, px, nl, self.n * nprob) + (nin[:nprob],)

    def step(self, blen, blimbs, nprob=1, transpose=False, sense=1, key=None, stream=None):
        """One exact simplex step on the device (slip_hip_factor_step): the selection of `ratio_test` on the same right-hand
        sides, then the new numerators x_i = (anum_best * xnum_i - xnum_best * anum_i) / det (entry best: xnum_best) over the
        new denominator d = anum_best, with no second solve.  Returns a StepResult; where best is -1 the problem's entries of
        x and its d are empty."""
        nprob = int(nprob)
        blen, blimbs, _ = _rhs(self.n, blen, blimbs, 2 * nprob if nprob >= 1 else nprob)
        key = _ratio_key(self.n, key)
        res = [np.zeros(max(nprob, 1), np.int32) for _ in range(4)]
        pl, px, nl = C.c_void_p(), C.c_void_p(), C.c_int64()
        ql, qx, qn = C.c_void_p(), C.c_void_p(), C.c_int64()
        rc = self.lib.slip_hip_factor_step(self.h, int(bool(transpose)), nprob, blen.ctypes.data, blimbs.ctypes.data, int(sense),
                                           None if key is None else key.ctypes.data, *[r.ctypes.data for r in res],
                                           C.byref(pl), C.byref(px), C.byref(nl), C.byref(ql), C.byref(qx), C.byref(qn),
                                           C.c_void_p(stream or 0))
        if rc:
            raise SlipError(rc, "slip_hip_factor_step")
        x = _take_slab(self.lib, pl, px, nl, self.n * nprob)
        d = _take_slab(self.lib, ql, qx, qn, nprob)
        return StepResult(*(r[:nprob] for r in res), x, d)

    def step_bounded(self, blen, blimbs, bounds, entering=None, nprob=1, transpose=False, sense=1, key=None, stream=None):
        """One bounded exact simplex step on the device (slip_hip_factor_step_bounded): the right-hand sides and index
        conventions of `ratio_test_bounded`, the definition of the module's `step_bounded` with d = det; no numerator crosses
        the host between the selection and the update.  Returns a BoundedStepResult."""
        nprob = int(nprob)
        blen, blimbs, _ = _rhs(self.n, blen, blimbs, 2 * nprob if nprob >= 1 else nprob)
        key = _ratio_key(self.n, key)
        head = [self.h, int(bool(transpose)), nprob, blen.ctypes.data, blimbs.ctypes.data]
        return _step_bounded_call(self.lib, self.lib.slip_hip_factor_step_bounded, "slip_hip_factor_step_bounded", head, self.n, nprob,
                                  bounds, entering, sense, key, stream)

    def step_bounded_ms(self):
        """device ms of the last step_bounded: [the selection's form passes, the selection, the scalars, the update]"""
        out = np.zeros(4, np.float64)
        self.lib.slip_hip_factor_step_bounded_ms(self.h, out.ctypes.data)
        return [float(v) for v in out]

    def step_bounded_paths(self):
        """the last step_bounded, as the module's `step_bounded_paths`"""
        out = np.zeros(20, np.int64)
        self.lib.slip_hip_factor_step_bounded_paths(self.h, out.ctypes.data)
        return [int(v) for v in out]

    def update_ms(self):
        """device ms of the last solve_update or step: [the classify, offset and form passes, the selection of a step]"""
        out = np.zeros(2, np.float64)
        self.lib.slip_hip_factor_update_ms(self.h, out.ctypes.data)
        return [float(v) for v in out]

    def update_paths(self):
        """the last solve_update or step, as the module's `pivot_update_paths`"""
        out = np.zeros(8, np.int64)
        self.lib.slip_hip_factor_update_paths(self.h, out.ctypes.data)
        return [int(v) for v in out]

    def price(self, M, blen, blimbs, nprob=1, sides=1, cost=None, sense=1, key=None, winners=False, stream=None):
        """Solve, multiply and select on the device (slip_hip_factor_price): b holds sides * nprob right-hand sides as
        `solve_transpose` takes them, M is a SparseMatrix with m == n whose columns are the candidates.  With y the
        numerators of the solve by row id over det, column j of M gives X_j = M(:,j)^T y_x - det * cost_c[j] (cost: None or
        (signed limb counts, limbs) of nprob * ncols entries) and, with sides=2, A_j = M(:,j)^T y_a.  sides=1: best is the j
        with the smallest sense * X_j / det (the reduced cost of column j is -X_j / det: sense=-1 is the most negative one);
        sides=2: the dual ratio test, `ratio_test`'s definition on (X, A).  Exact ties go to the smallest (key[j], j).
        Returns (best, nties, neligible, vsign), int32[nprob] each, vsign the sign of X_best / det; with winners=True also
        (wlen, wlimbs): X_best and A_best of problem c as entries 2c and 2c + 1 (sides=1: the second one empty), both empty
        where best is -1.  No numerator is downloaded otherwise."""
        nprob, sides = int(nprob), int(sides)
        ncols = M.ncols
        blen, blimbs, _ = _rhs(self.n, blen, blimbs, sides * nprob if nprob >= 1 and sides in (1, 2) else 0)
        if cost is None:
            g = (None, None, 0)
        else:
            glen, glimbs, gcap = _limb_arrays(*cost)
            if nprob >= 1 and glen.size != nprob * ncols:
                raise ValueError("price: cost must hold nprob*ncols entries")
            g = (glen.ctypes.data, glimbs.ctypes.data, gcap)
        key = _ratio_key(ncols, key)
        best, nties, nelig, vsign = (np.zeros(max(nprob, 1), np.int32) for _ in range(4))
        pl, px, nl = C.c_void_p(), C.c_void_p(), C.c_int64()
        outs = (C.byref(pl), C.byref(px), C.byref(nl)) if winners else (None, None, None)
        rc = self.lib.slip_hip_factor_price(self.h, M.h, sides, nprob, blen.ctypes.data, blimbs.ctypes.data, *g,
                                            int(sense), None if key is None else key.ctypes.data,
                                            best.ctypes.data, nties.ctypes.data, nelig.ctypes.data, vsign.ctypes.data,
                                            *outs, C.c_void_p(stream or 0))
        if rc:
            raise SlipError(rc, "slip_hip_factor_price")
        res = (best[:nprob], nties[:nprob], nelig[:nprob], vsign[:nprob])
        return res + _take_slab(self.lib, pl, px, nl, 2 * nprob) if winners else res

    def price_ms(self):
        """device ms of the last price by pass: [the record gather and the widths, the offset scans, the products, the
        selection] (the substitution: solve_transpose_ms)"""
        out = np.zeros(4, np.float64)
        self.lib.slip_hip_factor_price_ms(self.h, out.ctypes.data)
        return [float(v) for v in out]

    def price_paths(self):
        """the last price: the four counts of ratio_test_paths over its selections"""
        return _paths(self.lib.slip_hip_factor_price_paths, self.h)

    def price_states(self, M, blen, blimbs, state, weights=None, nprob=1, sides=1, cost=None, sense=1, key=None, winners=False,
                     stream=None):
        """Solve, multiply and select on the device with a state per column of M (slip_hip_factor_price_states): the
        operands, X_j and A_j of `price`, the states, weights and definition of the module's `price_select` with d = det.
        Returns (best, nties, neligible, vsign[, wlen, wlimbs]); nothing of y, X, A or the squares is downloaded otherwise."""
        nprob, sides = int(nprob), int(sides)
        ncols = M.ncols
        blen, blimbs, _ = _rhs(self.n, blen, blimbs, sides * nprob if nprob >= 1 and sides in (1, 2) else 0)
        if cost is None:
            g = (None, None, 0)
        else:
            glen, glimbs, gcap = _limb_arrays(*cost)
            if nprob >= 1 and glen.size != nprob * ncols:
                raise ValueError("price_states: cost must hold nprob*ncols entries")
            g = (glen.ctypes.data, glimbs.ctypes.data, gcap)
        keep, sargs = _states_args(ncols, state, weights, "price_states")
        key = _ratio_key(ncols, key)
        res = [np.zeros(max(nprob, 1), np.int32) for _ in range(4)]
        pl, px, nl = C.c_void_p(), C.c_void_p(), C.c_int64()
        outs = (C.byref(pl), C.byref(px), C.byref(nl)) if winners else (None, None, None)
        rc = self.lib.slip_hip_factor_price_states(self.h, M.h, sides, nprob, blen.ctypes.data, blimbs.ctypes.data, *g, *sargs,
                                                   int(sense), None if key is None else key.ctypes.data,
                                                   *[r.ctypes.data for r in res], *outs, C.c_void_p(stream or 0))
        return _bounded_results(self.lib, rc, "slip_hip_factor_price_states", res, nprob, winners, 2, pl, px, nl)

    def price_states_ms(self):
        """device ms of the last price_states: [the classify, offset and square passes, the selection] (the substitution:
        solve_transpose_ms)"""
        out = np.zeros(2, np.float64)
        self.lib.slip_hip_factor_price_states_ms(self.h, out.ctypes.data)
        return [float(v) for v in out]

    def price_states_paths(self):
        """the last price_states, as the module's `price_select_paths`"""
        out = np.zeros(8, np.int64)
        self.lib.slip_hip_factor_price_states_paths(self.h, out.ctypes.data)
        return [int(v) for v in out]

    def solve_transpose_ms(self):
        """(device ms of the last transposed solve's substitution kernels, ms of that call's view build: 0 when it was reused)"""
        view = C.c_double()
        ms = self.lib.slip_hip_factor_solve_transpose_ms(self.h, C.byref(view))
        return ms, view.value

    def pivots(self):
        """the pivot chain rho[0..K) only (signed limb counts, limbs): what the subtree farm exchanges"""
        i = self.info()
        K = i["K"]
        rholen = np.zeros(max(K, 1), np.int32)
        rho = np.zeros(max(i["l_limbs"], 1), np.uint64)
        cap = C.c_int64(rho.size)
        rc = self.lib.slip_hip_factor_download(self.h, None, None, None, None, None, None, None, None, None, None,
                                               rholen.ctypes.data, rho.ctypes.data, C.byref(cap), None)
        if rc:
            raise SlipError(rc, "slip_hip_factor_download")
        return rholen[:K], rho[:cap.value].copy()

    def rescale(self, scales, stream=None):
        """Subtree farm: multiply the committed columns by per-column big-integer scales on the device
        (slip_hip_factor_rescale): L(:,k), rho[k] by scales[k]; U entries by the scale of their row's pivot position."""
        lens, limbs = [], []
        for v in scales:
            a, l = abs(int(v)), 0
            while a:
                limbs.append(a & (2 ** 64 - 1)); a >>= 64; l += 1
            lens.append(-l if v < 0 else l)
        lens = np.array(lens, np.int32); limbs = np.array(limbs if limbs else [0], np.uint64)
        K = self.info()["K"]
        if len(lens) != K:
            raise ValueError(f"rescale needs one scale per committed column: {len(lens)} given, K = {K}")
        rc = self.lib.slip_hip_factor_rescale(self.h, int(len(lens)), lens.ctypes.data, limbs.ctypes.data, C.c_void_p(stream or 0))
        if rc:
            raise SlipError(rc, "slip_hip_factor_rescale")

    def solve_ms(self):
        return self.lib.slip_hip_factor_solve_ms(self.h)

    def close(self):
        if getattr(self, "h", None):
            self.lib.slip_hip_factor_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def factorize(n, Ap, Ai, Alen, Alimbs, q, pivot=3, tol=1.0, kmax=0, limb_cap=0, waves=0, check=True,
              lib_path=None, workers=0, lnz_hint=0, unz_hint=0, debug_flags=0):
    """One-shot SLIP_LU_factorize on the GPU; returns the canonical factor dict."""
    f = Factorization(n, Ap, Ai, Alen, Alimbs, q, pivot=pivot, tol=tol, limb_cap=limb_cap, waves=waves,
                      lib_path=lib_path, workers=workers, lnz_hint=lnz_hint, unz_hint=unz_hint, debug_flags=debug_flags)
    try:
        rc = f.run(kmax, check=check)
        out = f.download()
        out["status"] = rc
        return out
    finally:
        f.close()
