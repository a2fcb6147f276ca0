"""Shared by tests/test_emu_product.py (the emulator build) and tests/test_gpu_product.py (the product on the device): the
exact sparse products r = op(A) x - d b returned as signed big integers (slip_hip_factor_multiply on a handle,
slip_hip_matrix_* on a resident rectangular matrix).  The oracle is Python integers; every comparison is exact equality of
the returned slab (rlen, rlimbs), normalisation included.  lib_path None is the product library."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
from check_helpers import columns, residual, rhs_pair, slab, verdict
from conftest import load_case

B = 2 ** 32


def digits(v):
    return (abs(int(v)).bit_length() + 31) // 32


def same_slab(got, want_values, what=""):
    """the returned slab is exactly the normalised slab of the expected integers"""
    wlen, wlimbs = slab(want_values)
    assert np.array_equal(np.asarray(got[0], np.int64), wlen.astype(np.int64)), what
    assert np.array_equal(np.asarray(got[1], np.uint64), wlimbs), what


class Mat:
    """an m x ncols CSC of Python ints, entries as given (a repeated row of a column stays in the arrays)"""

    def __init__(self, m, ncols, cols):
        self.m, self.ncols, self.cols = m, ncols, cols             # cols[j]: list of (row, value) in entry order
        self.Ap = np.cumsum([0] + [len(c) for c in cols]).astype(np.int64)
        self.Ai = np.array([r for c in cols for r, _ in c], np.int32)
        self.vals = [v for c in cols for _, v in c]
        self.Alen, self.Alimbs = slab(self.vals)
        self.last = [dict(c) for c in cols]                        # the matrix that is multiplied: the LAST value wins

    def device(self, lib_path):
        import slip_lu_amd as sl
        return sl.SparseMatrix(self.m, self.ncols, self.Ap, self.Ai, self.Alen, self.Alimbs, lib_path=lib_path)

    def transposed(self):
        cols = [[] for _ in range(self.m)]
        for j, c in enumerate(self.last):
            for i, v in c.items():
                cols[i].append((j, v))
        return Mat(self.ncols, self.m, cols)

    def terms(self, transpose):
        """output row -> list of (a, index of x)"""
        rows = [[] for _ in range(self.ncols if transpose else self.m)]
        for j, c in enumerate(self.last):
            for i, v in c.items():
                rows[j if transpose else i].append((v, i if transpose else j))
        return rows

    def product(self, xs, bs=None, ds=None, transpose=False):
        """r_c = op(M) x_c - d_c b_c over all vectors, flat"""
        out = []
        for c, x in enumerate(xs):
            for i, row in enumerate(self.terms(transpose)):
                out.append(sum(a * x[k] for a, k in row) - (ds[c] * bs[c][i] if bs is not None else 0))
        return out

    def widths(self, xs, bs=None, ds=None, transpose=False):
        """W = max(max_e(|a_e| + |x_e|), |d| + |b_i|) + 1 of every item, as the kernel derives it"""
        out = []
        for c, x in enumerate(xs):
            for i, row in enumerate(self.terms(transpose)):
                w = max([digits(a) + digits(x[k]) for a, k in row] + [0])
                if bs is not None:
                    w = max(w, digits(ds[c]) + digits(bs[c][i]))
                out.append(w + 1)
        return out


def multiply(dev, xs, bs=None, ds=None, transpose=False):
    xlen, xlimbs = slab([v for x in xs for v in x])
    b = slab([v for bb in bs for v in bb]) if bs is not None else None
    d = slab(ds) if ds is not None else None
    return dev.multiply(xlen, xlimbs, nvec=len(xs), transpose=transpose, b=b, d=d)


# ---- 1. the synthetic corpus ----

TOP = B - 1                 # a one-digit entry with every bit set
X = 2 ** (32 * 62) - 12345  # 62 digits, the top digit all ones
BORDER_W = (64, 65, 128, 129, 192, 193, 256, 257, 300)


def corpus(wide_everywhere):
    """A 12 x 9 matrix and three vectors (x, b, d).  Row i <= 8 has its widest term in column i, a one-digit entry against
    x0[i] of BORDER_W[i] - 2 digits: vector 0 puts one item on each side of every class border and two on the memory path.
    Vector 2 makes rows 1..6 cancel two 63-digit terms down to 0, +1, -1, B^5, -B^5 and B^6 - 1.  Vector 1 is short (the
    entries of A are the longer operands).  Row 9 is empty, row 10 holds an explicit zero, column 3 repeats row 11.
    wide_everywhere: vectors 1 and 2 are wide in columns 7 and 8 too (more items on the memory path)."""
    rows = {
        0: {0: TOP},
        1: {0: 7, 1: 7},
        2: {0: 7, 2: -1},
        3: {0: 7, 3: -1},
        4: {0: 7, 4: -1},
        5: {0: 7, 5: -1},
        6: {0: 7, 6: -1},
        7: {7: TOP, 2: -(2 ** 70 + 9), 1: 2 ** 40 + 1},
        8: {8: -TOP, 7: 3, 3: 2 ** 33},
        9: {},
        10: {0: 0, 1: 2 ** 150 + 77, 2: 3},
        11: {3: -4, 5: 2},
    }
    cols = [[] for _ in range(9)]
    for i in sorted(rows):
        for j, v in rows[i].items():
            if (i, j) == (11, 3):
                cols[j].append((11, 99))                           # overwritten by the -4 that follows
            cols[j].append((i, v))
    m = Mat(12, 9, cols)
    x0 = [(-1) ** i * (2 ** (32 * (w - 2)) - 1 - i) for i, w in enumerate(BORDER_W)]
    x0[0] = X
    far = [2 ** (32 * 255) - 3, -(2 ** (32 * 290) + 1)] if wide_everywhere else [5, -6]
    x1 = [123, 2 ** 40 + 3, 0, -1, 2 ** 64, 0, -(2 ** 31), far[0], far[1]]
    x2 = [X, -X, 7 * X - 1, 7 * X + 1, 7 * X - B ** 5, 7 * X + B ** 5, 7 * X - (B ** 6 - 1), far[1] if wide_everywhere else 1, far[0] if wide_everywhere else 0]
    b0 = [3, -2 ** 40, 0, 1, 2, 3, 4, 5, 6, 0, 7, -8]
    b1 = [0, 1, -1, 2 ** 100, 0, 0, 5, 0, 0, -(2 ** 200 + 3), 0, 9]
    b2 = [2 ** 64 - 1, 0, 0, 0, 0, 0, 0, 1, -1, 17, 0, 2 ** 32]
    return m, [x0, x1, x2], [b0, b1, b2], [-3, 1, 2 ** 70 + 5]


def assert_corpus_shapes(m, xs, bs, ds, max_wide):
    """the corpus really holds every shape the tests are about (max_wide: the items above 256 digits allowed, None: any)"""
    W = m.widths(xs)
    r = m.product(xs)
    Wb = m.widths(xs, bs, ds)
    rb = m.product(xs, bs, ds)
    assert [W[i] for i in range(9)] == list(BORDER_W) == [Wb[i] for i in range(9)]
    wide = sum(1 for w in W if w > 256)
    assert wide >= 2 and (max_wide is None or wide <= max_wide) and sum(1 for w in Wb if w > 256) == wide
    adig = {digits(v) for v in m.vals}
    assert {1, 2, 3} <= adig and max(adig) >= 4 and 0 in adig                       # 1, 2, 3+ digits, an explicit zero
    pairs = [(digits(a), digits(xs[c][k])) for c in range(3) for row in m.terms(False) for a, k in row if a and xs[c][k]]
    assert any(la > lx for la, lx in pairs) and any(la < lx for la, lx in pairs)
    assert any(v > 0 for v in r) and any(v < 0 for v in r)
    v2 = r[24:36]
    assert v2[1:7] == [0, 1, -1, B ** 5, -B ** 5, B ** 6 - 1] and all(w in (64, 65) for w in W[25:31])      # wide terms cancelled
    for vals, ws in ((r, W), (rb, Wb)):                            # all of W - 1 digits, the top bit of the top digit set
        assert any(digits(v) == w - 1 and abs(v) >> (32 * (w - 1) - 1) for v, w in zip(vals, ws))
    assert any(digits(v) == w - 1 and abs(v) >> (32 * (w - 1) - 1) and w > 256 for v, w in zip(r, W))
    assert not m.terms(False)[9] and r[9] == 0 and W[9] == 1                        # an empty row, without b
    assert rb[9] == 0 and rb[12 + 9] == 2 ** 200 + 3 and rb[24 + 9] == -17 * (2 ** 70 + 5)   # with b = 0, and -d b alone
    assert any(v == 0 for x in xs for v in x)
    assert len(m.cols[3]) == len(m.last[3]) + 1 and m.last[3][11] == -4             # the repeated row
    assert any(digits(v) % 2 for x in xs for v in x) and any(digits(v) % 2 for v in r) and any(w % 2 for w in W)
    assert any(d < 0 for d in ds)


def check_corpus(lib_path, wide_everywhere):
    """both orientations of the corpus -- M x through the row view, (M^T)^T x through the column view of the transposed
    matrix -- with and without b, one vector and three"""
    m, xs, bs, ds = corpus(wide_everywhere)
    assert_corpus_shapes(m, xs, bs, ds, None if wide_everywhere else 2)
    mt = m.transposed()
    for mat, transpose in ((m, False), (mt, True)):
        dev = mat.device(lib_path)
        try:
            same_slab(multiply(dev, xs, transpose=transpose), m.product(xs), "three vectors")
            same_slab(multiply(dev, xs, bs, ds, transpose=transpose), m.product(xs, bs, ds), "three vectors, b and d")
            assert dev.multiply_ms() >= 0
            # one vector; in the other orientation of the same object the short vector 1, padded to its length
            same_slab(multiply(dev, xs[1:2], bs[1:2], ds[1:2], transpose=transpose), m.product(xs[1:2], bs[1:2], ds[1:2]), "one vector")
            y = [[5, -(2 ** 64), 0, 1, 2 ** 31, -7, 2 ** 100, 0, 3, -1, 2, 9]]
            same_slab(multiply(dev, y, transpose=not transpose), m.product(y, transpose=True), "the other view")
        finally:
            dev.close()


def check_groups(lib_path, monkeypatch):
    """a staging bound below one vector's need: every vector is its own group, the result is the same slab"""
    m, xs, bs, ds = corpus(False)
    monkeypatch.setenv("SLIP_HIP_PRODUCT_STAGE_KB", "1")
    dev = m.device(lib_path)
    try:
        same_slab(multiply(dev, xs, bs, ds), m.product(xs, bs, ds))
    finally:
        dev.close()


def check_thin(lib_path):
    """one row, and one column"""
    for m in (Mat(1, 4, [[(0, 3)], [], [(0, -(2 ** 64))], [(0, 1)]]), Mat(5, 1, [[(4, 2 ** 33), (0, -1), (2, 7)]])):
        dev = m.device(lib_path)
        try:
            for transpose in (False, True):
                nx, nout = (m.m, m.ncols) if transpose else (m.ncols, m.m)
                xs = [[(-1) ** (c + k) * (2 ** (40 * c + 3 * k) + k) for k in range(nx)] for c in range(3)]
                bs = [[(c - 1) * (k + 2 ** (70 * c)) for k in range(nout)] for c in range(3)]
                ds = [2, -1, 2 ** 64 + 1]
                for nvec in (1, 3):
                    same_slab(multiply(dev, xs[:nvec], transpose=transpose), m.product(xs[:nvec], transpose=transpose))
                    same_slab(multiply(dev, xs[:nvec], bs[:nvec], ds[:nvec], transpose=transpose),
                              m.product(xs[:nvec], bs[:nvec], ds[:nvec], transpose=transpose))
        finally:
            dev.close()


# ---- 2. on handles, goldens ----

def handle_width(cols, q, x):
    """the largest W of A(:,q) x over the rows, x by position"""
    return max(digits(a) + digits(x[p]) for p in range(len(q)) for a in cols[int(q[p])].values() if x[p]) + 1


def check_golden(lib_path, name, memory_path=False, **kw):
    import slip_lu_amd as sl
    _, fix = load_case(name)
    n, Ap, Ai, Alen, Alimbs, q = len(fix["q"]), fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"]
    cols = columns(n, Ap, Ai, oracle_lib.bigints(Alen, Alimbs))
    bs = rhs_pair(n)
    flat_b = [v for b in bs for v in b]
    b = slab(flat_b)
    f = sl.Factorization(n, Ap, Ai, Alen, Alimbs, q, lib_path=lib_path, **kw)
    try:
        f.run(0)
        det = oracle_lib.bigints(*f.pivots())[-1]
        xlen, xlimbs = f.solve(*b, nrhs=3)
        # A(:,q) xnum == det b entry by entry; minus det b: nothing is left, and nothing is returned for it
        same_slab(f.multiply(xlen, xlimbs, nvec=3), [det * v for v in flat_b], "multiply(solve(b))")
        rlen, rlimbs = f.multiply(xlen, xlimbs, nvec=3, b=b)
        assert not rlen.any() and rlen.size == 3 * n and rlimbs.size == 0
        assert f.multiply_ms() >= 0
        # the same transposed: b by position, x by row id
        tlen, tlimbs = f.solve_transpose(*b, nrhs=3)
        same_slab(f.multiply(tlen, tlimbs, nvec=3, transpose=True), [det * v for v in flat_b], "multiply(solve_transpose(b))")
        rlen, rlimbs = f.multiply(tlen, tlimbs, nvec=3, transpose=True, b=b)
        assert not rlen.any() and rlimbs.size == 0
        # one numerator of the middle vector perturbed: the exact residual, nonzero exactly where the check says
        x = oracle_lib.bigints(xlen, xlimbs)
        if memory_path:
            assert handle_width(cols, q, x[n:2 * n]) > 256, "the memory path (W > 256 digits) was not reached"
        p = max((t for t in range(n, 2 * n) if x[t]), key=lambda t: (digits(x[t]), t))
        y = list(x); y[p] += 2 ** 31
        want = []
        for c in range(3):
            xcol = [0] * n
            for t in range(n):
                xcol[int(q[t])] = y[c * n + t]
            want += residual(n, cols, xcol, det, bs[c])
        ylen, ylimbs = slab(y)
        same_slab(f.multiply(ylen, ylimbs, nvec=3, b=b), want, "the residual of a perturbed vector")
        ok, first, bad = f.check(*b, ylen, ylimbs, nrhs=3)
        assert not ok
        assert [(int(first[c]), int(bad[c])) for c in range(3)] == [verdict(want[c * n:(c + 1) * n]) for c in range(3)]
        assert want[:n] == [0] * n and want[2 * n:] == [0] * n and any(want[n:2 * n])
        # an explicit d: r = A(:,q) x - d b for any d
        same_slab(f.multiply(ylen[:n], ylimbs[:int(np.abs(ylen[:n].astype(np.int64)).sum())], b=slab(bs[0]), d=slab([-5])),
                  [det * v + 5 * v for v in bs[0]], "an explicit d")
    finally:
        f.close()


# ---- 3. lifecycle ----

def position_product(n, cols, q, x, transpose=False):
    """A(:,q) x by row (x by position), or A(:,q)^T x by position (x by row id)"""
    if transpose:
        return [sum(a * x[i] for i, a in cols[int(q[k])].items()) for k in range(n)]
    xcol = [0] * n
    for p in range(n):
        xcol[int(q[p])] = x[p]
    return residual(n, cols, xcol, 0, [0] * n)


def check_lifecycle(lib_path, name="gen_n40", **kw):
    import slip_lu_amd as sl
    _, fix = load_case(name)
    n, Ap, Ai, Alen, Alimbs, q = len(fix["q"]), fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"]
    vals = oracle_lib.bigints(Alen, Alimbs)
    cols = columns(n, Ap, Ai, vals)
    x = [(-1) ** t * (2 ** (9 * t) + t) if t % 5 else 0 for t in range(n)]
    bvec = [t - 7 for t in range(n)]
    xs, b = slab(x), slab(bvec)
    f = sl.Factorization(n, Ap, Ai, Alen, Alimbs, q, lib_path=lib_path, **kw)
    try:
        # before any column is factorised: the product alone, and with an explicit d
        for transpose in (False, True):
            same_slab(f.multiply(*xs, transpose=transpose), position_product(n, cols, q, x, transpose), "before run")
        same_slab(f.multiply(*xs, b=b, d=slab([3])), [v - 3 * w for v, w in zip(position_product(n, cols, q, x), bvec)])
        with pytest.raises(sl.SlipError) as e:                    # d = det does not exist yet
            f.multiply(*xs, b=b)
        assert e.value.code == -3
        f.run(0)
        fac = f.download()
        f.rewind(n // 2)
        for transpose in (False, True):
            same_slab(f.multiply(*xs, transpose=transpose), position_product(n, cols, q, x, transpose), "after rewind")
        with pytest.raises(sl.SlipError) as e:
            f.multiply(*xs, b=b)
        assert e.value.code == -3
        # a column replaced: the NEW matrix is multiplied, as a SparseMatrix of it does (x by column there)
        j = int(q[n // 3])
        new = {3: 2 ** 90 + 1, n - 1: -5, 0: 11}
        f.replace_column(j, list(new), list(new.values()))
        cols[j] = dict(new)
        nAp = np.cumsum([0] + [len(c) for c in cols]).astype(np.int64)
        nAi = np.array([r for c in cols for r in c], np.int32)
        nAlen, nAlimbs = slab([v for c in cols for v in c.values()])
        xcol = [0] * n
        for p in range(n):
            xcol[int(q[p])] = x[p]
        m1 = sl.SparseMatrix(n, n, nAp, nAi, nAlen, nAlimbs, lib_path=lib_path)
        m2 = sl.SparseMatrix(n, n, Ap, Ai, Alen, Alimbs, lib_path=lib_path)           # the old matrix, alive next to it
        try:
            got = f.multiply(*xs)
            same_slab(got, position_product(n, cols, q, x), "after replace_column")
            r1 = m1.multiply(*slab(xcol))
            assert np.array_equal(got[0], r1[0]) and np.array_equal(got[1], r1[1])
            same_slab(m2.multiply(*slab(xcol)), position_product(n, columns(n, Ap, Ai, vals), q, x), "the old matrix")
            same_slab(f.multiply(*xs, transpose=True), position_product(n, cols, q, x, True), "after replace_column, transposed")
        finally:
            m1.close(); m1.close()
            m2.close()
    finally:
        f.close()
    g = sl.Factorization.from_factors(fac, lib_path=lib_path, **{k: v for k, v in kw.items() if k in ("waves", "workers")})
    try:
        with pytest.raises(sl.SlipError) as e:                    # a handle around given factors holds no A
            g.multiply(*xs)
        assert e.value.code == -3
    finally:
        g.close()


# ---- 4. rejections: host-side verdicts, all SLIP_HIP_INCORRECT_INPUT (-3) ----

def check_rejections(lib_path):
    import slip_lu_amd as sl
    from slip_lu_amd import _lib
    lib = _lib.load(lib_path)
    m = Mat(3, 2, [[(0, 1), (2, -2)], [(1, 2 ** 64)]])
    xlen, xlimbs = slab([5, -(2 ** 64)])
    blen, blimbs = slab([1, 2 ** 64, 3])
    dlen, dlimbs = slab([2 ** 64 + 1])
    zlen, zlimbs = np.zeros(1, np.int32), np.zeros(1, np.uint64)
    pl, px, nl = C.c_void_p(), C.c_void_p(), C.c_int64()
    outs = (C.byref(pl), C.byref(px), C.byref(nl))
    X_, B_, D_, NONE = (xlen.ctypes.data, xlimbs.ctypes.data, xlimbs.size), (blen.ctypes.data, blimbs.ctypes.data, blimbs.size), \
        (dlen.ctypes.data, dlimbs.ctypes.data, dlimbs.size), (None, None, 0)

    def refused(fn, h):
        bad = [(h, 0, 0, *X_, *B_, *D_, *outs, None),                                # nvec < 1
               (None, 0, 1, *X_, *B_, *D_, *outs, None),                             # no object
               (h, 0, 1, None, X_[1], X_[2], *NONE, *NONE, *outs, None),             # NULL x
               (h, 0, 1, X_[0], None, X_[2], *NONE, *NONE, *outs, None),
               (h, 0, 1, *X_, *NONE, *NONE, None, outs[1], outs[2], None),           # NULL outputs
               (h, 0, 1, *X_, *NONE, *NONE, outs[0], None, outs[2], None),
               (h, 0, 1, *X_, *NONE, *NONE, outs[0], outs[1], None, None),
               (h, 0, 1, X_[0], X_[1], X_[2] - 1, *NONE, *NONE, *outs, None),        # slabs shorter than their lengths say
               (h, 0, 1, *X_, B_[0], B_[1], B_[2] - 1, *D_, *outs, None),
               (h, 0, 1, *X_, *B_, D_[0], D_[1], D_[2] - 1, *outs, None),
               (h, 0, 1, *X_, B_[0], None, B_[2], *D_, *outs, None),                 # counts without limbs
               (h, 0, 1, *X_, *NONE, *D_, *outs, None),                              # d without b
               (h, 0, 1, *X_, *B_, zlen.ctypes.data, zlimbs.ctypes.data, 1, *outs, None)]      # a zero d
        for args in bad:
            assert fn(*args) == -3, args[1:3]
        assert pl.value is None and px.value is None

    dev = m.device(lib_path)
    try:
        refused(lib.slip_hip_matrix_multiply, dev.h)
        assert lib.slip_hip_matrix_multiply(dev.h, 0, 1, *X_, *B_, *NONE, *outs, None) == -3        # b without d on a matrix
        with pytest.raises(ValueError):
            dev.multiply(xlen, xlimbs, transpose=True)            # three entries are needed there
        same_slab(dev.multiply(xlen, xlimbs, b=(blen, blimbs), d=(dlen, dlimbs)), m.product([[5, -(2 ** 64)]], [[1, 2 ** 64, 3]], [2 ** 64 + 1]))
    finally:
        dev.close()
    # a square matrix on a handle that was never run: the same verdicts, nothing factorised
    sq = Mat(3, 3, [[(0, 1), (2, -2)], [(1, 2 ** 64)], [(2, 5)]])
    f = sl.Factorization(3, sq.Ap, sq.Ai, sq.Alen, sq.Alimbs, np.arange(3, dtype=np.int32), lib_path=lib_path)
    try:
        xlen, xlimbs = slab([5, -(2 ** 64), 1])
        X_ = (xlen.ctypes.data, xlimbs.ctypes.data, xlimbs.size)
        refused(lib.slip_hip_factor_multiply, f.h)
    finally:
        f.close()
    # creation: missing arguments, empty shapes, a row outside the matrix
    h = C.c_void_p()
    args = (m.Ap.ctypes.data, m.Ai.ctypes.data, m.Alen.ctypes.data, m.Alimbs.ctypes.data)
    assert lib.slip_hip_matrix_create(None, 3, 2, *args) == -3
    for k in range(4):
        assert lib.slip_hip_matrix_create(C.byref(h), 3, 2, *[None if t == k else a for t, a in enumerate(args)]) == -3
    assert lib.slip_hip_matrix_create(C.byref(h), 0, 2, *args) == -3 and lib.slip_hip_matrix_create(C.byref(h), 3, 0, *args) == -3
    assert lib.slip_hip_matrix_create(C.byref(h), 2, 2, *args) == -3                  # row 2 of a 2 x 2 matrix
    assert h.value is None
    lib.slip_hip_matrix_destroy(None)
