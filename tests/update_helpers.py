"""Shared by tests/test_emu_update.py (the emulator build) and tests/test_gpu_update.py (the product on the device): the
rewind to column K (slip_hip_factor_rewind) and the replacement of a column of the resident A
(slip_hip_factor_replace_column), with the storage report slip_hip_factor_a_storage.  Ground truth is always the CPU
restatement (oracle_lib) on the matrix as it stands, or an existing golden -- never a second run of the code under test.
lib_path None is the product library."""
import ctypes as C
import random

import numpy as np
import pytest

import oracle_lib
from check_helpers import slab
from conftest import check_against_golden, load_case

FACTOR_KEYS = ("pinv", "Lp", "Li", "Llen", "Llimbs", "Up", "Ui", "Ulen", "Ulimbs", "rholen", "rholimbs")
WIDE = 2 ** 130 + 12345              # times a one-limb value: three limbs


class Mat:
    """A as a list of columns of (row, value) pairs in entry order, Python ints; a repeated row is kept as given"""

    def __init__(self, n, Ap, Ai, vals, q, pivot=3, tol=1.0):
        self.n, self.q, self.pivot, self.tol = n, np.array(q, np.int32), pivot, tol
        self.cols = [[(int(Ai[p]), int(vals[p])) for p in range(int(Ap[j]), int(Ap[j + 1]))] for j in range(n)]

    @classmethod
    def case(cls, name, pivot=None):
        entry, fix = load_case(name)
        n = len(fix["q"])
        m = cls(n, fix["Ap"], fix["Ai"], oracle_lib.bigints(fix["Alen"], fix["Alimbs"]), fix["q"],
                entry["pivot"] if pivot is None else pivot, entry["tol"])
        m.entry, m.fix = entry, fix
        return m

    def csc(self, canonical=False):
        """Ap, Ai, Alen, Alimbs; canonical: a repeated row once, with its LAST value, where that occurrence stands"""
        cols = [canon(c) for c in self.cols] if canonical else self.cols
        Ap = np.cumsum([0] + [len(c) for c in cols]).astype(np.int64)
        Ai = np.array([r for c in cols for r, _ in c], np.int32)
        Alen, Alimbs = slab([v for c in cols for _, v in c])
        return Ap, Ai, Alen, Alimbs

    def position(self, j):
        return int(np.where(self.q == j)[0][0])

    def handle(self, lib_path, **kw):
        import slip_lu_amd as sl
        return sl.Factorization(self.n, *self.csc(), self.q, pivot=self.pivot, tol=self.tol, lib_path=lib_path, **kw)

    def oracle(self, kmax=0):
        return oracle_lib.factorize(self.n, *self.csc(canonical=True), self.q, pivot=self.pivot, tol=self.tol, kmax=kmax)

    def oracle_solve(self, b):
        return oracle_lib.factorize_and_solve(self.n, *self.csc(canonical=True), self.q, b, pivot=self.pivot, tol=self.tol)

    def limbs(self):
        return sum((abs(v).bit_length() + 63) // 64 for c in self.cols for _, v in canon(c))

    def nnz(self):
        return sum(len(canon(c)) for c in self.cols)


def canon(col):
    last = {r: t for t, (r, _) in enumerate(col)}
    return [(r, v) for t, (r, v) in enumerate(col) if last[r] == t]


def same_factors(got, ref, what=""):
    """the downloaded factors, pivots, pinv and info are the oracle's"""
    assert got["K"] == ref["K"], (what, got["K"], ref["K"])
    for k in FACTOR_KEYS:
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(ref[k]).astype(np.int64)), (what, k)
    i = got["info"]
    assert (i["K"], i["lnz"], i["unz"], i["l_limbs"], i["u_limbs"]) == \
        (ref["K"], int(ref["Lp"][ref["K"]]), int(ref["Up"][ref["K"]]), len(ref["Llimbs"]), len(ref["Ulimbs"])), (what, i)


def empty_ref(n):
    """what a handle at column 0 serves (the oracle's kmax = 0 means all columns)"""
    ref = {k: np.zeros(0, np.int64) for k in FACTOR_KEYS}
    ref.update(n=n, K=0, Lp=np.zeros(1, np.int64), Up=np.zeros(1, np.int64), pinv=np.arange(n))
    return ref


def contested_positions(ref, K):
    """positions x >= K that the undo of columns n-1 .. K writes more than once (from the oracle's complete factorisation):
    by column x itself and by an earlier column c >= K whose pivot row stood at x -- where the smallest c has to win"""
    n = ref["n"]
    piv_row = np.argsort(ref["pinv"])
    pinv, rowperm = list(range(n)), list(range(n))
    writers = [set() for _ in range(n)]
    for k in range(n):
        r = int(piv_row[k])
        p, d = pinv[r], rowperm[k]
        rowperm[k], rowperm[p], pinv[r], pinv[d] = r, d, k, p
        if p == k:
            rowperm[k], pinv[r] = r, k
        if k >= K:
            writers[k].add(k); writers[p].add(k)
    return sum(len(w) > 1 for w in writers[K:])


def check_rewind_equals_run(lib_path, name, pivot, Ks=None, **kw):
    """complete, rewind(K): what the handle serves is the oracle's run to K; run() from there is the complete
    factorisation again.  Returns how many (K, position) pairs had more than one writer in the undo."""
    m = Mat.case(name, pivot)
    full = m.oracle()
    assert full["status"] == 0 and full["K"] == m.n
    contested = 0
    f = m.handle(lib_path, **kw)
    try:
        f.run()
        for K in (range(m.n + 1) if Ks is None else Ks):
            f.rewind(K)
            same_factors(f.download(), m.oracle(kmax=K) if K else empty_ref(m.n), (name, pivot, K))
            contested += contested_positions(full, K)
            assert f.run() == 0
        same_factors(f.download(), full, (name, pivot, "run again"))
    finally:
        f.close()
    return contested


def rhs(n):
    return [int(v) for v in oracle_lib.solve_rhs(n)]


def check_solves(f, m, what=""):
    """solve, check and the transposed solve on the handle against the oracle on the matrix m"""
    n, b = m.n, rhs(m.n)
    blen, blimbs = slab(b)
    want, det = m.oracle_solve(np.array(b, np.int64))
    xlen, xlimbs = f.solve(blen, blimbs)
    assert oracle_lib.bigints(xlen, xlimbs) == want, what
    ok, first, bad = f.check(blen, blimbs, xlen, xlimbs)
    assert ok and list(first) == [-1] and list(bad) == [0], what
    c = [((k * 40503) % 1999) - 999 for k in range(n)]
    clen, climbs = slab(c)
    z = oracle_lib.bigints(*f.solve_transpose(clen, climbs))
    cols = [dict(canon(col)) for col in m.cols]
    assert not any(sum(a * z[i] for i, a in cols[int(m.q[k])].items()) - det * c[k] for k in range(n)), what
    ok, first, bad = f.check_transpose(clen, climbs, *slab(z))
    assert ok and list(first) == [-1], what
    return want, det


def check_rewind_then_run(lib_path, name, K, **kw):
    """rewind(K), run(): the golden's factors; solve, check and the transposed solve (its view dropped and built again)"""
    m = Mat.case(name)
    f = m.handle(lib_path, **kw)
    try:
        f.run()
        check_solves(f, m, "before")
        f.rewind(K)
        assert f.info()["K"] == K
        with pytest.raises(Exception):
            f.solve(*slab(rhs(m.n)))                       # incomplete
        assert f.run() == 0
        check_against_golden(m.entry, m.fix, f.download(), counters=False)
        check_solves(f, m, "after")
    finally:
        f.close()


def new_content(m, j, kind):
    """a new column j of the given kind: [(row, value)], and the (lens, limbs) slab when the kind is about the slab form"""
    old = canon(m.cols[j])
    rows = [r for r, _ in old]
    free = [r for r in range(m.n) if r not in rows]
    if kind == "more":
        col = [(r, 3 * v + 1) for r, v in old] + [(r, 7 - 2 * r) for r in free[:3]]
    elif kind == "fewer":
        col = [(r, -v + 2) for r, v in old[:max(1, len(old) // 2)]]
    elif kind == "single":
        col = [(old[0][0], -5)]
    elif kind == "wide":
        col = [(r, (v + 1) * WIDE) for r, v in old]
    elif kind == "dup":
        col = [(old[0][0], 5)] + [(r, v + 3) for r, v in old[1:]] + [(old[0][0], -3)] + [(r, 11) for r in free[:1]]
    elif kind == "hizero":
        col = [(r, 2 * v - 1) for r, v in old]
        lens, limbs = [], []
        for t, (_, v) in enumerate(col):
            pad = 1 + t % 3                                  # high zero limbs behind the value's own
            l, x = slab([v])
            limbs += [int(w) for w in x] + [0] * pad
            lens.append((abs(int(l[0])) + pad) * (-1 if v < 0 else 1))
        return col, (np.array(lens, np.int32), np.array(limbs, np.uint64))
    else:
        raise ValueError(kind)
    return col, None


def nonsingular_content(m, j, kind):
    """new_content, moved to another row of the pattern until the oracle finds the new matrix nonsingular (the oracle is the
    reference: the choice is made on the CPU)"""
    col, sl = new_content(m, j, kind)
    keep = m.cols[j]
    for shift in range(m.n):
        m.cols[j] = [((r + shift) % m.n, v) for r, v in col]
        if m.oracle()["status"] == 0:
            got = m.cols[j]
            m.cols[j] = keep
            return got, sl
    raise AssertionError("no nonsingular variant")


def replace(f, m, j, col, sl=None):
    """on the handle and in the model"""
    if sl is None:
        f.replace_column(j, [r for r, _ in col], [v for _, v in col])
    else:
        f.replace_column(j, [r for r, _ in col], slab=sl)
    m.cols[j] = list(col)


def check_replace(lib_path, name, where, kind, **kw):
    """complete, replace the column at position 0 / n//2 / n-1, run: factors, pinv and a solve are the oracle's on the new
    matrix; the handle was rewound to the column's position and no further"""
    m = Mat.case(name)
    p = {"first": 0, "middle": m.n // 2, "last": m.n - 1}[where]
    j = int(m.q[p])
    col, sl = nonsingular_content(m, j, kind)
    f = m.handle(lib_path, **kw)
    try:
        f.run()
        xcap = f.info()["xcap_digits"]
        replace(f, m, j, col, sl)
        assert f.info()["K"] == p
        if kind == "wide":
            assert f.info()["xcap_digits"] > xcap           # the stride grew with the column
        same_factors(f.download(), m.oracle(kmax=p) if p else empty_ref(m.n), "rewound")
        assert f.run() == 0
        ref = m.oracle()
        assert ref["status"] == 0
        same_factors(f.download(), ref, (name, where, kind))
        check_solves(f, m, (name, where, kind))
        st = f.a_storage()
        assert (st["nnz"], st["limbs"]) == (m.nnz(), m.limbs())
    finally:
        f.close()


def check_replace_ahead(lib_path, name="gen_n40", **kw):
    """a column that has not been factorised yet (info.K <= p) is replaced without a rewind: the committed columns and the
    counters of their work stay"""
    m = Mat.case(name)
    K1 = m.n // 3
    f = m.handle(lib_path, **kw)
    try:
        f.run(K1)
        before = f.download()
        for p in (K1, m.n - 1):
            j = int(m.q[p])
            col, sl = nonsingular_content(m, j, "more")
            replace(f, m, j, col, sl)
            after = f.download()
            assert after["info"]["K"] == K1 and np.array_equal(after["counters"], before["counters"])
            same_factors(after, m.oracle(kmax=K1), "ahead")
        assert before["counters"][0] > 0
        assert f.run() == 0
        same_factors(f.download(), m.oracle(), "ahead, complete")
    finally:
        f.close()


def check_sequence(lib_path, name="gen_n40", steps=12, **kw):
    """successive replacements, each checked against the oracle on the matrix as it stands"""
    m = Mat.case(name)
    rng = random.Random(7)
    kinds = ["more", "fewer", "single", "wide", "dup", "hizero"]
    f = m.handle(lib_path, **kw)
    try:
        f.run()
        for s in range(steps):
            j = rng.randrange(m.n)
            col, sl = nonsingular_content(m, j, kinds[s % len(kinds)])
            replace(f, m, j, col, sl)
            assert f.info()["K"] == min(m.n, m.position(j))
            assert f.run() == 0
            same_factors(f.download(), m.oracle(), (s, j))
        check_solves(f, m, "sequence")
    finally:
        f.close()


def check_storage_bound(lib_path, name="test_mat", steps=64, **kw):
    """one column replaced again and again by four-limb values: the storage of A stays within twice its live content plus the
    initial allocation, the live figures are the model's, and the matrix is still the model's (oracle) along the way"""
    m = Mat.case(name)
    j = int(m.q[m.n // 2])
    rows = [r for r, _ in canon(m.cols[j])]
    f = m.handle(lib_path, **kw)
    try:
        st0 = f.a_storage()
        assert (st0["nnz"], st0["limbs"]) == (m.nnz(), m.limbs())
        caps = []
        for s in range(steps):
            col = [(r, (s + 2 + 3 * t) * 2 ** 200 + 17 * s + t + 1) for t, r in enumerate(rows)]
            replace(f, m, j, col)
            st = f.a_storage()
            assert (st["nnz"], st["limbs"]) == (m.nnz(), m.limbs()), s
            assert st["nnz"] <= st["nnz_cap"] <= 2 * st["nnz"] + st0["nnz_cap"], (s, st, st0)
            assert st["limbs"] <= st["limbs_cap"] <= 2 * st["limbs"] + st0["limbs_cap"], (s, st, st0)
            caps.append(st["limbs_cap"])
            if s % 16 == 15:
                assert f.run() == 0
                same_factors(f.download(), m.oracle(), s)
        assert any(b < a for a, b in zip(caps, caps[1:])), caps      # the slab was compacted on the way
    finally:
        f.close()


def check_singular_repaired(lib_path, name="gen_n40", **kw):
    """a column made a copy of another: SLIP_HIP_SINGULAR at the reference's column; replaced by an independent one: complete,
    the golden"""
    m = Mat.case(name)
    p1, p2 = m.n // 4, (2 * m.n) // 3
    j1, j2 = int(m.q[p1]), int(m.q[p2])
    good = list(m.cols[j2])
    f = m.handle(lib_path, **kw)
    try:
        f.run()
        replace(f, m, j2, canon(m.cols[j1]))
        ref = m.oracle()
        assert ref["status"] == -2 and ref["K"] < m.n
        assert f.run(check=False) == -2
        got = f.download()
        assert got["info"]["K"] == ref["K"] and got["info"]["status"] == -2
        same_factors(got, ref, "singular")
        replace(f, m, j2, good)
        assert f.run() == 0
        check_against_golden(m.entry, m.fix, f.download(), counters=False)
        check_solves(f, m, "repaired")
    finally:
        f.close()


def check_certificate(lib_path, name="gen_n40", **kw):
    """after a replacement the certificate tests the NEW matrix: it accepts the new solve and reports SLIP_HIP_INCORRECT for
    the numerators obtained before, with the same b"""
    m = Mat.case(name)
    b = rhs(m.n)
    blen, blimbs = slab(b)
    j = int(m.q[m.n // 2])
    col, sl = nonsingular_content(m, j, "more")
    f = m.handle(lib_path, **kw)
    try:
        f.run()
        x0len, x0limbs = f.solve(blen, blimbs)
        assert f.check(blen, blimbs, x0len, x0limbs)[0]
        replace(f, m, j, col, sl)
        assert f.run() == 0
        want, det = check_solves(f, m, "new")
        # on the CPU: the old numerators do not solve the new system
        x0 = oracle_lib.bigints(x0len, x0limbs)
        cols = [dict(canon(c)) for c in m.cols]
        r = [-det * v for v in b]
        for pos in range(m.n):
            for i, a in cols[int(m.q[pos])].items():
                r[i] += a * x0[pos]
        bad_rows = [i for i, v in enumerate(r) if v]
        assert bad_rows and x0 != want
        ok, first, bad = f.check(blen, blimbs, x0len, x0limbs)
        assert not ok and int(first[0]) == bad_rows[0] and int(bad[0]) == len(bad_rows)
    finally:
        f.close()


def check_q_tail(lib_path, name="gen_n40", **kw):
    """position p moved to the end: the oracle's result for that order; a tail with a repeated or a foreign id is refused and
    the handle still serves the old result"""
    import slip_lu_amd as sl
    m = Mat.case(name)
    p = m.n // 3
    f = m.handle(lib_path, **kw)
    try:
        f.run()
        old = m.oracle()
        tail = list(m.q[p:])
        for bad_tail in (tail[:-1] + tail[:1], tail[:-1] + [int(m.q[0])], [m.n] + tail[1:], [-1] + tail[1:]):
            with pytest.raises(sl.SlipError) as e:
                f.rewind(p, q_tail=bad_tail)
            assert e.value.code == -3
            same_factors(f.download(), old, "refused tail")
        check_solves(f, m, "refused tail")
        newq = np.concatenate([m.q[:p], m.q[p + 1:], m.q[p:p + 1]]).astype(np.int32)
        f.rewind(p, q_tail=newq[p:])
        m.q = newq
        assert f.info()["K"] == p
        assert f.run() == 0
        same_factors(f.download(), m.oracle(), "moved to the end")
        check_solves(f, m, "moved to the end")                # the check's views follow the new order
        f.rewind(m.n, q_tail=[])                             # an empty tail: nothing to do
        same_factors(f.download(), m.oracle(), "empty tail")
    finally:
        f.close()


def check_refusals(lib_path, name="test_mat", **kw):
    """every refused call is SLIP_HIP_INCORRECT_INPUT (-3) and leaves the handle as it was"""
    import slip_lu_amd as sl
    m = Mat.case(name)
    n = m.n
    j = int(m.q[1])
    rows = np.array([r for r, _ in canon(m.cols[j])], np.int32)
    lens, limbs = slab([v * WIDE for _, v in canon(m.cols[j])])
    f = m.handle(lib_path, **kw)
    try:
        f.run(n // 2)
        lib, vp = f.lib, C.c_void_p
        calls = [lambda: f.rewind(-1), lambda: f.rewind(n // 2 + 1), lambda: f.rewind(n),
                 lambda: f.replace_column(j, [], []),                                     # nz < 1
                 lambda: f.replace_column(j, [0, n], [1, 2]), lambda: f.replace_column(j, [-1], [1]),
                 lambda: f.replace_column(-1, [0], [1]), lambda: f.replace_column(n, [0], [1])]
        for call in calls:
            with pytest.raises(sl.SlipError) as e:
                call()
            assert e.value.code == -3
        # a capacity short of what the counts say
        assert lib.slip_hip_factor_replace_column(f.h, j, int(rows.size), rows.ctypes.data, lens.ctypes.data, limbs.ctypes.data,
                                                  int(limbs.size) - 1, None) == -3
        assert f.info()["K"] == n // 2
        same_factors(f.download(), m.oracle(kmax=n // 2), "after the refusals")
        assert f.run() == 0
        check_against_golden(m.entry, m.fix, f.download(), counters=False)
        fac = f.download()
    finally:
        f.close()
    g = sl.Factorization.from_factors(fac, lib_path=lib_path)          # no A, no swap log behind this handle
    try:
        for call in (lambda: g.rewind(0), lambda: g.rewind(n), lambda: g.replace_column(j, [0], [1]), g.a_storage):
            with pytest.raises(sl.SlipError) as e:
                call()
            assert e.value.code == -3
        b = rhs(n)
        assert oracle_lib.bigints(*g.solve(*slab(b))) == m.oracle_solve(np.array(b, np.int64))[0]
    finally:
        g.close()
