"""Built operands for the column update x_i <- (hist(x_i) * rho_jn - L_m * x_j) / rho_{jn-1} at the edges of its width classes.

Small matrices (q = identity, pivot = DIAGONAL) put chosen operands into chosen updates, as tests/test_emu_raw_fill.py does for
the raw fill-in.  Every factorisation is held against two references: oracle_lib.factorize (bit for bit, counters included)
and a dense fraction-free elimination in Python integers (`dense_elimination`), which shares no code with either.

The info record has no per-class counters, so the INTENT of a case is checked here: `trace` replays the left-looking sweep in
Python integers and restates, for every update and history item, what the kernel derives from the operands' bit lengths --
slip_ipge_plan, the lane condition of ref_lu_pipe_cols.h, the Wn rule of slip_history_wave -- and `check_intent` asserts that
each labelled update lands in the class its case names.  A case that drifts off its edge fails there."""
import functools
from fractions import Fraction

import numpy as np

import oracle_lib
from test_emu_batch_commit import FACTOR_KEYS
from test_emu_raw_fill import DIAGONAL, _seed, csc, wide

B = 1 << 32
SINGULAR = -2           # SLIP_SINGULAR, SLIP_HIP_SINGULAR
EDGES = (64, 128, 192, 256)


def nbits(v):
    return abs(v).bit_length()


def ndig(v):
    return (nbits(v) + 31) >> 5


def ctz(v):
    return (v & -v).bit_length() - 1


def ones(b):
    return (1 << b) - 1


def up32(z):
    return (z + 31) >> 5


def width_class(w):
    """the register class slip_ipge_wave / slip_history_wave pick for a working width of w digits"""
    for c, e in enumerate(EDGES):
        if w <= e:
            return "reg%d" % (c + 1)
    return "mem"


# ---------------------------------------------------------------------------------------------------------------------------
# reference 2: dense fraction-free elimination, plain Python integers
# ---------------------------------------------------------------------------------------------------------------------------
def dense_elimination(n, cols):
    """M(k)[i][j] = (M(k-1)[i][j] * M(k-1)[p][k-1] - M(k-1)[i][k-1] * M(k-1)[p][j]) / rho_{k-2}; the pivot of column k is the
    diagonal when it is nonzero, else the nonzero entry of smallest magnitude among the rows that are not pivotal yet (the cases
    leave exactly one).  Returns dict(K, L {(row, k)}, U {(k, column)}, rho [..], pinv [..])."""
    M = [[cols.get(j, {}).get(i, 0) for j in range(n)] for i in range(n)]
    free, prev, L, U, rho, pinv = list(range(n)), 1, {}, {}, [], [-1] * n
    for k in range(n):
        cand = [i for i in free if M[i][k]]
        if not cand:
            break
        p = k if k in cand else min(cand, key=lambda i: abs(M[i][k]))
        assert p == k or [abs(M[i][k]) for i in cand].count(abs(M[p][k])) == 1, "the smallest candidate must be unique"
        for i in free:
            L[i, k] = M[i][k]
        for j in range(k, n):
            U[k, j] = M[p][j]
        rho.append(M[p][k]); pinv[p] = k; free.remove(p)
        for i in free:
            for j in range(k + 1, n):
                num = M[i][j] * M[p][k] - M[i][k] * M[p][j]
                assert num % prev == 0
                M[i][j] = num // prev
        prev = M[p][k]
    return dict(K=len(rho), L=L, U=U, rho=rho, pinv=pinv)


def solve_numerators(n, cols, b):
    """x = det * A^-1 b in Fraction arithmetic (Gauss-Jordan on the dense matrix); det from dense_elimination"""
    M = [[Fraction(cols.get(j, {}).get(i, 0)) for j in range(n)] + [Fraction(b[i])] for i in range(n)]
    for k in range(n):
        p = next(i for i in range(k, n) if M[i][k] != 0)
        M[k], M[p] = M[p], M[k]
        M[k] = [v / M[k][k] for v in M[k]]
        for i in range(n):
            if i != k and M[i][k] != 0:
                f = M[i][k]
                M[i] = [a - f * c for a, c in zip(M[i], M[k])]
    det = dense_elimination(n, cols)["rho"][-1]
    out = [M[i][n] * det for i in range(n)]
    assert all(v.denominator == 1 for v in out)
    return [int(v) for v in out]


# ---------------------------------------------------------------------------------------------------------------------------
# the plan, restated
# ---------------------------------------------------------------------------------------------------------------------------
def ipge_plan(xi, hi, xj, Lm, rho, jn):
    """slip_ipge_plan: xi the target as stored (history tag hi), xj the finalised source, Lm the L entry, rho the pivots so far.
    Returns dict(W, W1, W2, hist, hdiv, bnum)."""
    has_d = jn >= 1
    bd = zd = 0
    if has_d:
        bd, zd = nbits(rho[jn - 1]), ctz(rho[jn - 1])
    hist = xi != 0 and has_d and hi < jn - 1
    hdiv = hist and hi > -1
    bh = zh = 0
    if hdiv:
        bh, zh = nbits(rho[hi]), ctz(rho[hi])
    bxp = 0 if not xi else (nbits(xi) if not hist else (nbits(xi) + bd - bh + 1 if hdiv else nbits(xi) + bd))
    b1b = bxp + nbits(rho[jn]) if xi else 0
    b2b = nbits(Lm) + nbits(xj)
    bnum = max(b1b, b2b) + 1
    bq = bnum - bd + 1 if has_d else bnum
    W = (bq + 1 + 31) >> 5                          # + sign bit
    W1 = W + (up32(zd) if has_d else 0)
    W2 = W1 + (up32(zh) if hdiv else 0)
    return dict(W=W, W1=W1, W2=W2, hist=hist, hdiv=hdiv, bnum=bnum)


def update_class(xi, hi, xj, Lm, rho, jn, raw):
    """where one update of the worker's sweep is computed: 'raw' (slip_fill_raw), 'lane' (the u128 path of ref_lu_pipe_cols.h:
    every operand of at most 2 digits and bnum <= 126), or the register class / memory path of slip_ipge_wave from W2"""
    if raw and xi == 0:
        return "raw", None
    pl = ipge_plan(xi, hi, xj, Lm, rho, jn)
    D = rho[jn - 1] if jn >= 1 else 0
    small = ndig(xj) <= 2 and ndig(rho[jn]) <= 2 and ndig(D) <= 2 and ndig(Lm) <= 2 and ndig(xi) <= 2
    if small and pl["bnum"] <= 126 and (not pl["hdiv"] or ndig(rho[hi]) <= 2):
        return "lane", pl
    return width_class(pl["W2"]), pl


def history_class(x, m, d):
    """x * m / d (d None: no division): 'small' (slip_history_small: every operand of at most 2 digits) or the class of Wn"""
    if ndig(x) <= 2 and ndig(m) <= 2 and (d is None or ndig(d) <= 2):
        return "small", None
    bq = nbits(x) + nbits(m)
    Wn = (bq + 31) >> 5
    if d is not None:
        Wn = ((bq - nbits(d) + 1 + 31) >> 5) + up32(ctz(d))
    return width_class(Wn), Wn


def trace(n, cols):
    """The left-looking sweep (q = identity; diagonal pivot, else the smallest) in Python integers, recording
    upd[(k, i, jn)] = (class, plan) for every update and his[(k, i)] = (class, Wn) for every history item that finishes a row
    of column k (a source's own finalisation is his[(k, j)] too).  Its values are held against dense_elimination."""
    rho, Lcol, perm, pinv = [], [], [], {}
    upd, his = {}, {}
    for k in range(n):
        x = dict(cols.get(k, {})); h = {i: -1 for i in x}
        done = -1
        while True:
            srcs = [pinv[i] for i in x if i in pinv and pinv[i] > done]
            if not srcs:
                break
            jn = done = min(srcs)
            j = perm[jn]
            for i in Lcol[jn]:
                if i not in x:
                    x[i] = 0; h[i] = -1
            if x[j] == 0:
                continue
            raw = h[j] == -1 and jn >= 1 and ndig(x[j]) <= 2
            a = x[j]
            if h[j] < jn - 1:
                d = rho[h[j]] if h[j] >= 0 else None
                his[k, j] = history_class(x[j], rho[jn - 1], d)
                x[j] = x[j] * rho[jn - 1] // (d if d is not None else 1)
            for i, Lm in Lcol[jn].items():
                if i == j or Lm == 0:
                    continue
                upd[k, i, jn] = update_class(x[i], h[i], x[j], Lm, rho, jn, raw)
                if raw and x[i] == 0:
                    x[i] = -a * Lm
                else:
                    y = x[i]
                    if y and jn >= 1 and h[i] < jn - 1:
                        y = y * rho[jn - 1] // (rho[h[i]] if h[i] >= 0 else 1)
                    num = y * rho[jn] - Lm * x[j]
                    assert jn == 0 or num % rho[jn - 1] == 0
                    x[i] = num // rho[jn - 1] if jn >= 1 else num
                h[i] = jn
        free = [i for i in x if i not in pinv]
        for i in free:
            if x[i] and k >= 1 and h[i] < k - 1:
                d = rho[h[i]] if h[i] >= 0 else None
                his[k, i] = history_class(x[i], rho[k - 1], d)
                x[i] = x[i] * rho[k - 1] // (d if d is not None else 1)
        cand = [i for i in free if x[i]]
        if not cand:
            break
        p = k if k in cand else min(cand, key=lambda i: abs(x[i]))
        rho.append(x[p]); perm.append(p); pinv[p] = k
        Lcol.append({i: x[i] for i in free})
    return dict(K=len(rho), upd=upd, his=his, rho=rho, Lcol=Lcol, pinv=pinv)


class Case:
    """one matrix and what its entries are there for: want_upd {(k, i, jn): (class, {plan word: value})},
    want_his {(k, i): (class, Wn or None)}, zeros [(row, k)] entries that must be stored as explicit zeros"""

    def __init__(self, name, n, cols, one_limb=False, K=None):
        self.name, self.n, self.cols, self.one_limb = name, n, cols, one_limb
        self.K = n if K is None else K
        self.want_upd, self.want_his, self.zeros, self.want_max = {}, {}, [], None

    def __repr__(self):
        return self.name


def check_intent(case):
    """every labelled update and history item is in the class its case names"""
    t = trace(case.n, case.cols)
    d = reference(case)["dense"]
    assert t["K"] == d["K"] == case.K, (case, t["K"], d["K"])
    for k in range(t["K"]):
        assert t["rho"][k] == d["rho"][k], (case, k)
        for i, v in t["Lcol"][k].items():
            assert v == d["L"][i, k], (case, i, k)
    assert case.want_upd or case.want_his, case
    for key, (cls, words) in case.want_upd.items():
        assert key in t["upd"], (case, key, "no such update")
        got_cls, pl = t["upd"][key]
        assert got_cls == cls, (case, key, got_cls, cls, pl)
        for w, v in words.items():
            got = width_class(pl[w[4:]]) if w.startswith("cls_") else pl[w]
            assert got == v, (case, key, w, got, v, pl)
    if case.want_max is not None:
        assert max(t["upd"][key][1]["W2"] for key in case.want_upd if t["upd"][key][1]) == case.want_max, (case, case.want_max)
    for key, (cls, Wn) in case.want_his.items():
        assert key in t["his"], (case, key, "no such history item")
        assert t["his"][key][0] == cls and (Wn is None or t["his"][key][1] == Wn), (case, key, t["his"][key], cls, Wn)
    for i, k in case.zeros:
        assert i in t["Lcol"][k] and t["Lcol"][k][i] == 0, (case, i, k)
    return t


# ---------------------------------------------------------------------------------------------------------------------------
# running a case against the two references
# ---------------------------------------------------------------------------------------------------------------------------
_REF = {}


def reference(case):
    """both references of a case, computed once and shared by every run of it"""
    if case.name not in _REF:
        arrays = csc(case.n, case.cols)
        q = np.arange(case.n, dtype=np.int32)
        _REF[case.name] = dict(arrays=arrays, q=q, oracle=oracle_lib.factorize(case.n, *arrays, q, pivot=DIAGONAL),
                               dense=dense_elimination(case.n, case.cols))
    return _REF[case.name]


def _columns(K, p, idx, lens, limbs):
    """stored columns -> [{id: value}] of K columns"""
    vals = oracle_lib.bigints(lens, limbs)
    return [{int(idx[m]): vals[m] for m in range(int(p[k]), int(p[k + 1]))} for k in range(K)]


def check_case(lib_path, case, waves, workers, seed, weak=0, **kw):
    """factorise on the emulator (lib_path) or the device (None) and hold the result against both references"""
    import slip_lu_amd as sl
    ref = reference(case)
    lib = _seed(lib_path, seed, weak) if lib_path else None
    try:
        got = sl.factorize(case.n, *ref["arrays"], ref["q"], pivot=DIAGONAL, waves=waves, workers=workers, lib_path=lib_path,
                           check=False, **kw)
    finally:
        if lib:
            lib.slip_emu_set_weak(0)
    orc, dense = ref["oracle"], ref["dense"]
    # 1. the CPU restatement, bit for bit
    assert got["K"] == orc["K"] == case.K, (got["K"], orc["K"], case.K)
    want_status = 0 if case.K == case.n else SINGULAR
    assert got["status"] == orc["status"] == want_status, (got["status"], orc["status"])
    for k in FACTOR_KEYS:
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(orc[k]).astype(np.int64)), k
    info = got["info"]
    if case.K == case.n:        # (a singular run's counters stop at the last committed column; the oracle's include the abandoned one)
        assert info["n_upd"] == int(orc["counters"][0]), (info["n_upd"], orc["counters"][0])
        assert info["limb_macs"] == int(orc["counters"][7]), (info["limb_macs"], orc["counters"][7])
    # 2. the dense elimination: every stored entry, explicit zeros included, and nothing nonzero left out
    K = got["K"]
    pinv = [int(p) for p in got["pinv"]]
    for i in range(case.n):
        if dense["pinv"][i] >= 0:
            assert pinv[i] == dense["pinv"][i], (i, pinv[i], dense["pinv"][i])
    assert oracle_lib.bigints(got["rholen"], got["rholimbs"]) == dense["rho"]
    Lc = _columns(K, got["Lp"], got["Li"], got["Llen"], got["Llimbs"])
    Uc = _columns(K, got["Up"], got["Ui"], got["Ulen"], got["Ulimbs"])
    for k in range(K):
        for i, v in Lc[k].items():
            assert v == dense["L"][i, k], ("L", i, k)
        for i, v in Uc[k].items():
            assert v == dense["U"][pinv[i], k], ("U", pinv[i], k)
    for (i, k), v in dense["L"].items():
        assert v == 0 or Lc[k].get(i) == v, ("L entry missing", i, k)
    for (p, j), v in dense["U"].items():
        if j < K:
            assert v == 0 or {pinv[i]: u for i, u in Uc[j].items()}.get(p) == v, ("U entry missing", p, j)
    for i, k in case.zeros:
        assert Lc[k].get(i, 1) == 0, ("explicit zero", i, k)
    return got


def solve_check(lib_path, case, b, waves, workers, seed):
    """one forward/back solve on the case's factors; numerators against Fraction arithmetic"""
    import slip_lu_amd as sl
    ref = reference(case)
    if lib_path:
        _seed(lib_path, seed)
    blen, blimbs = csc(1, {0: {i: v for i, v in enumerate(b) if v}})[2:]
    dense_len = np.zeros(case.n, np.int32)
    dense_len[[i for i, v in enumerate(b) if v]] = blen
    f = sl.Factorization(case.n, *ref["arrays"], ref["q"], pivot=DIAGONAL, waves=waves, workers=workers, lib_path=lib_path)
    try:
        f.run(0)
        xlen, xlimbs = f.solve(dense_len, blimbs)
    finally:
        f.close()
    assert oracle_lib.bigints(xlen, xlimbs) == solve_numerators(case.n, case.cols, b)


# ---------------------------------------------------------------------------------------------------------------------------
# Family A: level 0, no divisor: x_i * rho_0 - L_i0 * x_0 with the four operands given directly
# ---------------------------------------------------------------------------------------------------------------------------
def _grid(name, rho0, rowL, colx0, cells, one_limb=False):
    """Column 0 holds rho0 and the L entries of the target rows; columns 1.. hold x_0 in row 0, +-1 on the diagonal and the
    targets.  The target rows come after every such column and no column has another source, so L(t, c) is the update's own
    result (for c >= 2 behind a history item x * rho_{c-1} / rho_0 with rho_{c-1} = +-rho_0).  A cell without a target is a
    fill-in from source position 0, which the raw path does not take."""
    nc, nr = len(colx0), len(rowL)
    n = 1 + nc + nr
    cols = {j: {j: 1} for j in range(n)}
    cols[0] = {0: rho0}
    for r, Lv in enumerate(rowL):
        cols[0][1 + nc + r] = Lv
    for c, x0 in enumerate(colx0):
        cols[1 + c] = {0: x0, 1 + c: -1 if c % 2 else 1}
    for (r, c), v in cells.items():
        cols[1 + c][1 + nc + r] = v
    case = Case(name, n, cols, one_limb)
    case.at = lambda r, c: (1 + c, 1 + nc + r, 0)          # (k, i, jn) of cell (r, c)
    return case


def family_a_ones(T, S, neg=False, cls=None, full=True, signs16=True):
    """rho_0 = +-(2^b - 1).  Rows 0, 1: L = +-(2^c - 1) against columns x_0 = +-(2^d - 1) with targets +-(2^a - 1), a + b = c + d
    = S: both products have exactly S bits, the bound; with opposite product signs the sum has S + 1 = bnum bits and fills the
    W digits up to the sign bit (S = 32 T - 2).  Four columns: all eight sign combinations of x_i, L and x_0, every (s1, s2)
    twice (signs16; with the negative rho_0 of another case all sixteen); else the two columns with x_0 > 0: every (s1, s2)
    once.  Row 2 against the last column: exact cancellation x_i = a c, rho_0 = b d, L = a b, x_0 = c d, the zero kept as an entry.
    The rest of row 2 and of that column are empty targets: fill-ins from source position 0 with wide sources.  full: the
    cancellation and the fill-ins are labelled too (their bounds lie up to four bits below S, which keeps them in W = T only
    at the top of T's range)."""
    one_limb = S <= 128
    b = S // 2
    b -= b % 2                                     # 2^b - 1 = (2^(b/2) - 1)(2^(b/2) + 1)
    a = S - b
    c, d = (b, a) if one_limb else (a + 3, b - 3)  # another split of the same S
    fb, fd = ones(b // 2), ones(b // 2) + 2
    rho0 = -fb * fd if neg else fb * fd
    fa, fc = (wide(10, 31), wide(20, 32)) if one_limb else (wide((a - 2) // 2, 31), wide(a - 2 - (a - 2) // 2, 32))
    rowL = [ones(c), -ones(c), -fa * fb if neg else fa * fb]
    nsc = 4 if signs16 else 2
    colx0 = [ones(d), -ones(d), ones(d), -ones(d), fc * fd] if signs16 else [ones(d), ones(d), fc * fd]
    cells = {(r, col): ones(a) * (1 if col < nsc // 2 else -1) for r in range(2) for col in range(nsc)}
    cells[2, nsc] = fa * fc
    case = _grid("A-ones-W%d-S%d%s" % (T, S, "-neg" if neg else ""), rho0, rowL, colx0, cells, one_limb)
    cls = cls or width_class(T)
    words = {"bnum": S + 1} if one_limb else {"bnum": S + 1, "W2": T, "W": T}
    for r in range(2):
        for col in range(nsc):
            case.want_upd[case.at(r, col)] = (cls, words)
    case.zeros.append((case.at(2, nsc)[1], case.at(2, nsc)[0]))
    if full:
        rest = "lane" if one_limb else cls
        for r, col in ((2, nsc), (2, 0), (2, 1)):
            case.want_upd[case.at(r, col)] = (rest, {})
    return case


def family_a_pow(T, neg=False):
    """rho_0 = +-B^q, x_i = +-B^p, p + q = T - 1 (the bound is 32 (p + q) + 2 bits: W = W2 = T).  Rows 0, 1: L = +-(B^(p+q) - 1)
    against x_0 = +-1: the products are one apart, same signs leave 1 (a borrow run that collapses the whole width), opposite
    signs 2 B^(p+q) - 1.  Rows 2, 3: L = +-1: B^(p+q) -+ 1, the borrow crosses every lane and every register boundary.
    Row 4 against column 2: an empty target, a source of 70 bits and an all-ones L entry whose product has 32 T - 2 bits."""
    p = (T - 1) // 2
    q = T - 1 - p
    rho0 = -(B ** q) if neg else B ** q
    rowL = [B ** (p + q) - 1, -(B ** (p + q) - 1), 1, -1, -ones(32 * T - 72)]
    colx0 = [1, -1, wide(70, 34)]
    cells = {(r, c): B ** p * (-1 if c else 1) for r in range(4) for c in range(2)}
    case = _grid("A-pow-W%d%s" % (T, "-neg" if neg else ""), rho0, rowL, colx0, cells)
    for r in range(4):
        for c in range(2):
            case.want_upd[case.at(r, c)] = (width_class(T), {"W2": T})
    case.want_upd[case.at(4, 2)] = (width_class(T), {"W2": T})
    return case


def family_a_pow_one_limb(neg=False):
    """the same shapes in the lane: x_i = +-2^60, rho_0 = +-2^62, L x_0 = 2^122 - 1 = (2^61 - 1)(2^61 + 1), and L x_0 = +-1"""
    rho0 = -(1 << 62) if neg else 1 << 62
    rowL = [ones(61), -ones(61), 1, -1]
    colx0 = [(1 << 61) + 1, -((1 << 61) + 1), 1, -1]
    cells = {(r, c): (1 << 60) * (-1 if (r + c) % 3 == 0 else 1) for r in range(4) for c in range(4)}
    case = _grid("A-pow-lane%s" % ("-neg" if neg else ""), rho0, rowL, colx0, cells, True)
    for r in range(4):
        for c in range(4):
            case.want_upd[case.at(r, c)] = ("lane", {})
    return case


A_WIDTHS = (63, 64, 65, 128, 129, 192, 193, 256, 257, 300)


@functools.lru_cache(None)
def family_a():
    """{class: [cases]}: every edge width at the top of its range (S = 32 T - 2: the result reaches the sign bit), the first
    width past each edge (and 64) also at the bottom of its range (S = 32 (T - 1) - 1: bnum + 1 = 32 (T - 1) + 1, where the sign
    bit alone asks for the T-th digit: one bit over the edge), the negative rho_0 (the other eight of the sixteen sign
    combinations) at one width per class, and the one-limb cases at bnum = 126 (the lane's
    last) and 127 (the first wave item)"""
    out = {}
    for T in A_WIDTHS:
        s16 = T in EDGES + (300,)
        cases = [family_a_ones(T, 32 * T - 2, signs16=s16), family_a_pow(T)]
        if T - 1 in EDGES or T == 64:
            cases.append(family_a_ones(T, 32 * (T - 1) - 1, full=False, signs16=False))
        if s16:
            cases += [family_a_ones(T, 32 * T - 2, neg=True), family_a_pow(T, neg=True)]
        out.setdefault(width_class(T), []).extend(cases)
    out["lane"] = [family_a_ones(4, 125, cls="lane"), family_a_ones(4, 125, neg=True, cls="lane"),
                   family_a_ones(4, 126, cls="reg1"), family_a_ones(4, 126, neg=True, cls="reg1"),
                   family_a_pow_one_limb(), family_a_pow_one_limb(neg=True)]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# Family B: level 1, chosen divisor: the quotient is d * (A_ik * A_11 - A_i1 * A_1k)
# ---------------------------------------------------------------------------------------------------------------------------
def _largest(lo, hi, pred):
    """the largest v in [lo, hi] with pred(v), pred being true up to some point and false beyond it"""
    assert pred(lo), "nothing fits"
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if pred(mid):
            lo = mid
        else:
            hi = mid - 1
    return lo


def family_b_matrix(name, d, mb, one_limb=False):
    """Column 0 is its diagonal d alone: rho_0 = d, rho_1 = m d, L_i1 = A_i1 d with A_11 = m of mb bits.  Columns 2..5 bring
    A_1k in row 1 (the source at position 1) and targets in the rows behind every column, so L(i, k) is the quotient d * minor
    (for k >= 3 behind a history item x * rho_{k-1} / rho_1 with rho_{k-1} = +-rho_1).  Every entry has about mb bits:
      column 2: A_1k = m + 1 against row 6 (A_i1 = m - 1, target m): minor +1, the widest operands of the matrix
      column 3: A_1k = m - 1 against row 6 (target m - 2): minor -1
      column 4: A_1k = c e   against row 7 (A_i1 = -a b, target -a c, m = b e): minor 0, kept as an explicit zero
      column 5: A_1k = v     against row 8 (A_i1 = (u m - (2^kb - 1)) / v, target u): minor 2^kb - 1, kb a multiple of 32 when wide
    Every other cell with a target holds a wide random value; the cells without one are fill-ins from a multi-limb source."""
    fb, fe = wide(mb // 2, 41), wide(mb - mb // 2, 49)
    m = fb * fe
    a, c = wide(mb - mb // 2, 43) * fb, wide(mb // 2, 44) * fe
    kb = mb // 2 if one_limb else 32 * max((2 * mb - 40) // 32, 1)
    v = wide(mb, 48)
    while _gcd(m, v) != 1:
        v += 2
    u = (ones(kb) * pow(m, -1, v)) % v
    assert (u * m - ones(kb)) % v == 0
    rows = [m - 1, -a, (u * m - ones(kb)) // v]
    n = 9
    cols = {j: {j: 1} for j in range(n)}
    cols[0] = {0: d}
    cols[1] = {1: m}
    for r, val in enumerate(rows):
        cols[1][6 + r] = val
    cols[2] = {1: m + 1, 2: 1, 6: m, 7: -wide(mb, 45)}
    cols[3] = {1: m - 1, 3: -1, 6: m - 2, 8: wide(mb - 1, 46)}
    cols[4] = {1: c, 4: 1, 7: -(a // fb) * (c // fe)}
    cols[5] = {1: v, 5: -1, 8: u, 6: -wide(mb - 2, 47)}
    case = Case(name, n, cols, one_limb)
    case.zeros.append((7, 4))
    return case


def _gcd(a, b):
    while b:
        a, b = b, a % b
    return a


def family_b_case(tag, d, T, cls=None):
    """the matrix whose widest update (minor +1) works at W2 = T digits, at the top of T's range so that the other minors, a few
    bits narrower, work at T digits too; cls: the class the case names (default: T's).  One limb: rho_1, the L entries and the
    finalised sources fill their 64 bits (mb + bits(d) + 2 = 64)."""
    one_limb = cls == "lane"
    if one_limb:
        case = family_b_matrix("B-%s-lane" % tag, d, 62 - nbits(d), True)
    else:
        def fits(mb):
            c = family_b_matrix("", d, mb)
            upd = trace(c.n, c.cols)["upd"]
            return max(upd[key][1]["W2"] for key in B_CELLS) <= T
        case = family_b_matrix("B-%s-W%d" % (tag, T), d, _largest(34, 16 * T + 64, fits))
    cls = cls or width_class(T)
    for key in B_CELLS:
        case.want_upd[key] = (cls, {"hist": True, "hdiv": False})
    if not one_limb:
        case.want_max = T                                        # the widest of them works at exactly T digits
    # an empty target: a fill-in from a multi-limb source, or the raw path where A_1k = m + 1 fits one limb
    case.want_upd[2, 8, 1] = ("raw" if ndig(case.cols[2][1]) <= 2 else cls, {})
    return case


# (column, row, source position) of the minors +1, -1, 0, 2^kb - 1 and of a wide random one
B_CELLS = ((2, 6, 1), (3, 6, 1), (4, 7, 1), (5, 8, 1), (2, 7, 1))


# divisor, the width its case works at: every register class and the memory path get an even divisor with ctz >= 32 (wr_shr /
# wb_copy_shr through whole digits) and one with ctz < 32 (the funnel shift alone)
B_DIVISORS = (
    ("odd", 0xC0FFEE11, 64), ("odd-neg", -0xC0FFEE11, 65),
    ("ctz1", 2 * wide(40, 51), 64), ("ctz31", wide(50, 52) << 31, 128), ("ctz32", -wide(45, 53) << 32, 64),
    ("ctz33", wide(30, 54) << 33, 128), ("ctz63", -wide(70, 55) << 63, 192), ("ctz64", wide(33, 56) << 64, 256),
    ("ctz65", wide(64, 57) << 65, 257),
    ("B1", B, 65), ("B2", -(B ** 2), 66), ("B63", B ** 63, 129), ("B127", B ** 127, 257), ("B140", B ** 140, 300),
    ("Bm1-40", B ** 40 - 1, 128), ("even-wide", wide(1500, 58) << 5, 192), ("even-wide-neg", -wide(2100, 59) << 7, 256),
    ("even-wide-mem", wide(900, 60) << 30, 300),
)
B_ONE_LIMB = (("odd", 0x10001), ("odd-neg", -0xFFFF), ("ctz1", 6), ("ctz31", 3 << 31), ("ctz32", -(5 << 32)), ("B1", B))


@functools.lru_cache(None)
def family_b():
    out = {}
    for tag, d, T in B_DIVISORS:
        out.setdefault(width_class(T), []).append(family_b_case(tag, d, T))
    out["lane"] = [family_b_case(tag, d, 4, cls="lane") for tag, d in B_ONE_LIMB]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# Family C: a history update with a division inside the update, and as an item of its own
# ---------------------------------------------------------------------------------------------------------------------------
def family_c_matrix(name, r0, st, su, bx, one_limb=False):
    """rho_0 = r0 (even), rho_1 = a11 r0, rho_2 = a22 rho_1.  Rows 6, 7 are in L(:,0) and row 6 in L(:,2) too; neither is in
    L(:,1).  Column 3 holds x_0 and x_2: source 0 touches rows 6 and 7 (history tag 0), source 2 then updates row 6 with
    hist(x_6) = x_6 rho_1 / rho_0 inside the update (hdiv: W2 = W1 + digits of ctz(rho_0)), and row 7, which no later source
    touches, is finished by a history item x_7 rho_2 / rho_0.  st, su: bits of L(6,0) and L(7,0); bx: bits of the entries."""
    n = 8
    cols = {j: {j: 1} for j in range(n)}
    a11, a22 = (3, -5) if one_limb else (wide(bx, 71), -wide(bx, 72))
    cols[0] = {0: r0, 6: wide(st, 73), 7: -wide(su, 74)}
    cols[1] = {1: a11}
    cols[2] = {2: a22, 6: wide(bx, 75)}
    cols[3] = {0: -wide(bx, 76), 2: wide(bx, 77) if not one_limb else 7, 3: 1, 6: wide(bx, 78)}
    cols[4] = {0: wide(bx, 79), 4: -1}            # rows 6 and 7 again, both finished by history items
    return Case(name, n, cols, one_limb)


def family_c_case(E):
    """edge E: the update of row 6 in column 3 has W and W1 in the class that ends at E and W2 = E + 1 in the next; row 7
    is finished by a history item of Wn = E + 1 digits whose quotient has E - 1 (column 3), row 6 of column 4 by one of
    Wn <= E"""
    r0 = wide(90, 81) << 64                        # ctz(rho_0) = ctz(rho_1) = 64: two digits each
    bx = 40

    def upd_fits(st):
        c = family_c_matrix("", r0, st, 40, bx)
        return trace(c.n, c.cols)["upd"][3, 6, 2][1]["W2"] <= E + 1
    st = _largest(40, 32 * E, upd_fits)

    def his_fits(su):
        c = family_c_matrix("", r0, st, su, bx)
        return trace(c.n, c.cols)["his"][3, 7][1] <= E + 1
    c = family_c_matrix("C-edge%d" % E, r0, st, _largest(40, 32 * E, his_fits), bx)
    nxt = width_class(E + 1)
    c.want_upd[3, 6, 2] = (nxt, {"W": E - 3, "W1": E - 1, "W2": E + 1, "hdiv": True, "cls_W1": width_class(E), "cls_W": width_class(E)})
    c.want_his[3, 7] = (nxt, E + 1)
    c.want_his[4, 6] = (width_class(E), None)
    return c


def family_c_one_limb():
    """the same in one limb: every operand of exactly 2 digits, the update in the lane and the items in slip_history_small"""
    c = family_c_matrix("C-lane", 3 << 33, 18, 19, 17, one_limb=True)
    c.want_upd[3, 6, 2] = ("lane", {"hdiv": True})
    c.want_his[3, 7] = ("small", None)
    c.want_his[4, 7] = ("small", None)
    t = trace(c.n, c.cols)
    for v in (t["rho"][0], t["rho"][2], t["Lcol"][3][7], c.cols[0][7] * c.cols[3][0]):
        assert ndig(v) == 2, v
    return c


@functools.lru_cache(None)
def family_c():
    out = {width_class(E + 1): [family_c_case(E)] for E in EDGES}
    out["lane"] = [family_c_one_limb()]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# Family D: zeros that change the control flow
# ---------------------------------------------------------------------------------------------------------------------------
def family_d_matrix(name, bits, singular=False):
    """rho_0 = b e; rows 1, 5, 6 are in L(:,0) with L = a_r b; a column with x_0 = c e cancels the target a_r c exactly.
      column 3: row 1 cancels: the source at position 1 is zero and is skipped; row 8 of L(:,1) stays an explicit zero
      column 4: row 6 cancels, row 1 does not: source 1 then updates the zero row 6 (which is tagged and was touched)
      column 5: the diagonal cancels: the pivot moves to row 7; column 7 takes row 5
      column 5 (singular): its entries in rows 5 and 6 both cancel and nothing else is left: SLIP_SINGULAR at K = 5"""
    one = bits <= 32
    w = (lambda nb, s: wide(nb, s))
    fb, fe, fc = w(bits, 91), w(bits, 92), w(bits, 93)
    ar = {1: w(bits, 94), 5: -w(bits, 95), 6: w(bits, 96), 8: -w(bits, 97)}
    n = 10
    cols = {j: {j: w(max(bits // 2, 3), 100 + j)} for j in range(n)}
    cols[0] = {0: fb * fe, 1: ar[1] * fb, 5: ar[5] * fb, 6: ar[6] * fb}
    cols[1] = {1: w(bits, 98), 6: -w(bits, 99), 8: w(bits, 113)}
    cols[3] = {0: fc * fe, 1: ar[1] * fc, 3: 7}
    cols[4] = {0: -fc * fe, 1: w(bits, 110), 4: -3, 6: -ar[6] * fc}
    cols[5] = {0: fc * fe, 5: ar[5] * fc, 7: w(bits, 111)}
    cols[7] = {5: -w(bits, 112), 7: 11}
    K = n
    if singular:
        # rows 1, 5 and 6 all cancel in column 5: source 1 is skipped, rows 5 .. 9 hold nothing; the columns before it are as above
        cols[5] = {0: fc * fe, 1: ar[1] * fc, 5: ar[5] * fc, 6: ar[6] * fc}
        K = 5
    c = Case(name, n, cols, one, K)
    c.zeros.append((8, 3))
    return c


def family_d_case(bits, singular):
    name = "D-%s%s" % ("lane" if bits <= 32 else "bits%d" % bits, "-singular" if singular else "")
    c = family_d_matrix(name, bits, singular)
    cls = "lane" if bits <= 32 else None
    t = trace(c.n, c.cols)
    assert (3, 6, 1) not in t["upd"] and (3, 8, 1) not in t["upd"], "a zero source is skipped"
    wide_cls = cls or width_class(ndig(fbits(bits)))
    c.want_upd[3, 1, 0] = (wide_cls, {})          # cancels; later the source that is skipped
    c.want_upd[4, 6, 0] = (wide_cls, {})          # cancels; later a target
    c.want_upd[4, 6, 1] = (cls or t["upd"][4, 6, 1][0], {})
    c.want_upd[5, 5, 0] = (wide_cls, {})          # the diagonal cancels
    assert t["Lcol"][3][8] == 0
    if singular:
        c.want_upd[5, 6, 0] = (wide_cls, {})
        assert t["K"] == 5
    else:
        assert t["Lcol"][5][5] == 0 and t["pinv"][7] == 5 and t["pinv"][5] > 5
    return c


def fbits(bits):
    """the bound of the cancelling updates of family D: four factors of `bits` bits and the sign"""
    return 1 << (4 * bits + 2)


D_BITS = (15, 1040)         # one limb; about 130 digits in the cancelling updates


@functools.lru_cache(None)
def family_d():
    out = {}
    for bits in D_BITS:
        key = "lane" if bits <= 32 else width_class(ndig(fbits(bits)))
        out[key] = [family_d_case(bits, False), family_d_case(bits, True)]
    return out


FAMILIES = {"A": family_a, "B": family_b, "C": family_c, "D": family_d}


def cases_of(families, one_limb=None):
    """the cases of the families as pytest parameters, id = family-class-case; one_limb: only those (True) or only the others"""
    import pytest
    out = []
    for f in families:
        for cls, cases in FAMILIES[f]().items():
            for c in cases:
                if one_limb is None or c.one_limb == one_limb:
                    out.append(pytest.param(c, id="%s-%s-%s" % (f, cls, c.name)))
    return out


def case_named(family, name):
    return next(c for cases in FAMILIES[family]().values() for c in cases if c.name == name)


def edge_rhs(case, k):
    """a right-hand side that repeats column k of the matrix (the forward solve is that column's sweep), with an entry in row 0
    on top so that the back substitution has something to do"""
    b = [case.cols[k].get(i, 0) for i in range(case.n)]
    b[0] += 5
    return b


# Family E: the Family B matrices whose column 2 (minor +1, the widest update) is solved for
E_CASES = ("B-ctz1-lane", "B-ctz33-W128", "B-ctz63-W192", "B-even-wide-neg-W256", "B-ctz65-W257")
