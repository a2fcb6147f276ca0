"""Fill-in from an untouched source entry (ref_lu_pipe.h, slip_fill_raw): a row that is still zero gets x[i] = -a_j * L(i,jn)
when the source entry a_j has not been updated by any earlier source -- no product with rho, no division.  On the CPU
emulation of the kernel source, bit for bit against the CPU restatement (oracle_lib.factorize) or the reference's goldens;
`raw_fills` says how many rows took the path, and the constructed cases know that number."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
from conftest import ROOT, check_against_golden, load_case
from test_emu_batch_commit import FACTOR_KEYS, GOLDEN_RUNS

EMU = os.path.join(ROOT, "tests", "emu", "libslip_emu.so")
FARM = os.path.join(ROOT, "tests", "emu", "libslip_emu_farm.so")
DIAGONAL = 1            # SLIP_DIAGONAL: with q = identity and a nonzero diagonal the pivot of column k is row k


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "libslip_emu.so"])
    return EMU


@pytest.fixture(scope="module")
def emu_farm_lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "libslip_emu_farm.so"])
    return FARM


def _seed(path, seed, weak=0):
    lib = ctypes.CDLL(path)
    lib.slip_emu_set_seed.argtypes = [ctypes.c_ulonglong]
    lib.slip_emu_set_seed(seed)
    lib.slip_emu_set_weak(weak)
    return lib


def csc(n, cols):
    """cols: {column: {row: python int of any size}} -> (Ap, Ai, Alen, Alimbs), signed 64-bit limb counts"""
    Ap, Ai, lens, limbs = [0], [], [], []
    for j in range(n):
        for i in sorted(cols.get(j, {})):
            v = cols[j][i]
            m, nl = abs(v), (abs(v).bit_length() + 63) // 64
            Ai.append(i)
            lens.append(nl if v > 0 else -nl)
            limbs.extend((m >> (64 * t)) & (2 ** 64 - 1) for t in range(nl))
        Ap.append(len(Ai))
    return (np.array(Ap, dtype=np.int64), np.array(Ai, dtype=np.int32), np.array(lens, dtype=np.int32),
            np.array(limbs, dtype=np.uint64))


def wide(bits, seed):
    """a deterministic odd integer of exactly `bits` bits"""
    rng = np.random.RandomState(seed)
    v = 0
    for _ in range((bits + 31) // 32):
        v = (v << 32) | int(rng.randint(0, 2 ** 32, dtype=np.uint64))
    return (v & ((1 << bits) - 1)) | (1 << (bits - 1)) | 1


def expected_raw_fills(n, cols):
    """The count at pattern level, for q = identity and diagonal pivots, of a matrix without numerical cancellation: a source
    at position jn >= 1 is raw when its row is an entry of the column as given, of one limb, that no earlier source of the
    column reached; it fills every row of L(:,jn) below the diagonal that the column has not reached yet."""
    Lpat, total = {}, 0
    for k in range(n):
        x = {i: "raw" for i in cols.get(k, {})}
        for jn in range(k):
            if jn not in x:
                continue
            raw = x[jn] == "raw" and jn >= 1 and abs(cols[k][jn]) < 2 ** 64
            for i in Lpat[jn]:
                if i != jn:
                    total += raw and i not in x
                    x[i] = "upd"
        Lpat[k] = sorted(i for i in x if i >= k)
    return total


def check_constructed(lib_path, n, cols, want, waves, workers, seed, weak=0, **kw):
    import slip_lu_amd as sl
    Ap, Ai, Alen, Alimbs = csc(n, cols)
    q = np.arange(n, dtype=np.int32)
    lib = _seed(lib_path, seed, weak) if lib_path else None       # (no library path: the product library on the device)
    try:
        got = sl.factorize(n, Ap, Ai, Alen, Alimbs, q, pivot=DIAGONAL, waves=waves, workers=workers, lib_path=lib_path, check=False, **kw)
    finally:
        if lib:
            lib.slip_emu_set_weak(0)
    ref = oracle_lib.factorize(n, Ap, Ai, Alen, Alimbs, q, pivot=DIAGONAL)
    assert got["K"] == ref["K"] == n, (got["K"], ref["K"])
    for k in FACTOR_KEYS:
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(ref[k]).astype(np.int64)), k
    assert list(got["pinv"]) == list(range(n))
    info = got["info"]
    assert info["n_upd"] == int(ref["counters"][0])
    assert info["raw_fills"] == want, (info["raw_fills"], want)
    return info


# L entries of every width class of the short path, with the edges of the classes.  The product has digits(L) + digits(a) 32-bit
# digits.  Up to 64 limbs of L (40 .. 4064 bits here) the streaming lane multiplies (slip_fill_raw_lane); longer entries are wave
# items: 5000 .. 6112 bits in register class 3 (<= 192 digits), 7000 and 8160 bits in class 4 (<= 256), 9000 bits through memory.
# A short entry becomes a wave item only where the row has no room for the lane's 2 * (limbs + 1) digits: case_row_nearly_full.
WIDTHS = (40, 1000, 2016, 3000, 4064, 5000, 6112, 7000, 8160, 9000)


BASE_FILLS = 11 + 9 + 10 + 9


def base_matrix(rho0, a_pos, a_neg):
    """n = 16.  Column 0 is its diagonal rho0 alone, so L(i,1) = rho0 * A(i,1): rows 4.. of column 1 carry the wide entries,
    signs alternating.  Columns 2.. bring untouched entries in row 1 (source position 1, divisor rho[0] = rho0) and row 2."""
    n = 16
    cols = {j: {j: 7 + 2 * j} for j in range(n)}
    cols[0] = {0: rho0}
    cols[1] = {1: 5, 2: -9, 3: 11}
    for t, bits in enumerate(WIDTHS):
        cols[1][4 + t] = wide(bits, 100 + t) * (1 if t % 2 else -1)
    # raw source at position 1, one digit, positive; every row of L(:,1) below row 2 is still zero
    cols[2] = {1: a_pos, 2: 13}
    # the same source row, value between 2^32 and 2^64, negative; rows 5 and 8 hold values (zero and nonzero targets mixed);
    # row 2, filled in by it, is the next source: it is not raw
    cols[3] = {1: a_neg, 3: 17, 5: 123456789, 8: -wide(300, 7)}
    # raw source at position 2 (divisor rho[1], two sources later than the scatter), one digit, negative
    cols[4] = {2: -a_pos, 4: wide(70, 9)}
    # raw source at position 3 whose rho[2] is long by now; 64-bit value
    cols[5] = {3: -a_neg, 5: 19}
    return n, cols


def case_position_zero():
    """a source at position 0 has no division to save and is not counted; the untouched source behind it at position 2 is"""
    n = 8
    cols = {j: {j: 3 + j} for j in range(n)}
    cols[0] = {0: -4, 3: wide(3000, 1), 4: -wide(100, 2)}
    cols[2] = {2: 9, 5: wide(2500, 3), 6: 77}
    cols[3] = {0: 21, 3: 5}                    # source 0 fills row 4: general path (jn == 0)
    cols[4] = {2: -6, 4: 11}                   # row 2 is not in L(:,0): untouched at position 2, fills rows 5 and 6
    assert expected_raw_fills(n, cols) == 2
    return n, cols, 2


def case_cancelled_row():
    """a row that an earlier update made exactly zero (len == 0, tag set, history 0) is filled in like a fresh one"""
    n = 8
    cols = {j: {j: 3 + j} for j in range(n)}
    cols[0] = {0: -6, 4: 5}
    cols[1] = {1: 7, 4: wide(2100, 5), 5: -wide(90, 6)}
    # source 0: x[4] = 10 * rho[0] - L(4,0) * x[0] = 10 * (-6) - 5 * (-12) = 0; row 1 is not in L(:,0) and stays untouched
    cols[3] = {0: -12, 1: 1 << 40, 3: 5, 4: 10}
    return n, cols, 2                          # rows 4 (cancelled before) and 5


def case_multi_limb_source():
    """an untouched entry wider than one limb is not carried (the rule of slip_fill_raw): same factors, nothing counted"""
    n = 8
    cols = {j: {j: 3 + j} for j in range(n)}
    cols[1] = {1: -7, 4: wide(2100, 5), 5: -wide(90, 6)}
    cols[3] = {1: wide(65, 8), 3: 5}
    return n, cols, 0


def case_row_nearly_full():
    """An L entry of 15 digits in rows of 16 (inputs of at most 4 digits give the smallest row stride): the lane path wants
    2 * (8 + 1) = 18 digits and leaves the row to the wave item, whose product of 15 digits fits.  rho[2] has 384 bits,
    L(5,3) = A(5,3) * rho[2] and L(6,3) 464; the untouched -3 in row 3 of column 4 fills rows 5 and 6."""
    n = 8
    cols = {j: {j: 3 + j} for j in range(n)}
    cols[0] = {0: wide(128, 21)}
    cols[1] = {1: -wide(128, 22)}
    cols[2] = {2: wide(128, 23)}
    cols[3] = {3: 3, 5: wide(80, 24), 6: -wide(80, 25)}
    cols[4] = {3: -3, 4: 11}
    assert expected_raw_fills(n, cols) == 2
    return n, cols, 2


def case_long_column():
    """a source column of more than SLIP_WORK_CAP (512) entries is drained in several passes: the raw value goes with each"""
    n = 540
    cols = {j: {j: 3 + j % 11} for j in range(n)}
    cols[1] = {i: (wide(70, i) if i % 3 else -wide(40, i)) for i in range(1, n)}
    cols[1][1] = -5
    cols[n - 1] = {1: -(2 ** 33 + 1), n - 1: 3}
    # column n-1: rows 2 .. n-2 of L(:,1) are zero (row n-1 holds the diagonal entry); the columns between have no source
    assert expected_raw_fills(n, cols) == n - 3
    return n, cols, n - 3


def case_widths_and_signs(rho0):
    """every register class and the memory path, a below 2^32 and between 2^32 and 2^64, the four sign combinations of a_j and
    L_m; mixed zero and nonzero targets; a second source that is a fill"""
    n, cols = base_matrix(rho0, 0xF00DF00D, -0x1234567890ABCDEF)
    # by hand: L(:,1) has rows 2..13 below the diagonal; column 2 holds a value in row 2 (11 fills), column 3 in rows 3, 5 and 8 (9);
    # column 4's source row 2 is untouched: L(:,2) has rows 3..13, row 4 holds a value (10); column 5's source row 3: L(:,3) has
    # rows 4..13, row 5 holds a value (9)
    assert expected_raw_fills(n, cols) == BASE_FILLS
    return n, cols, BASE_FILLS


RHO0 = (3, -3, 6 << 33, -(5 << 2))          # rho[jn-1] positive / negative / even (ctz 34 and 2)
SMALL_CASES = (case_position_zero, case_cancelled_row, case_multi_limb_source)


@pytest.mark.parametrize("rho0", RHO0)
def test_raw_fill_widths_and_signs(emu_lib, rho0):
    n, cols, want = case_widths_and_signs(rho0)
    check_constructed(emu_lib, n, cols, want, 2, 5, 1)


@pytest.mark.parametrize("case", SMALL_CASES, ids=lambda c: c.__name__)
def test_raw_fill_small_cases(emu_lib, case):
    n, cols, want = case()
    check_constructed(emu_lib, n, cols, want, 2, 4, 3)


def test_raw_fill_into_a_row_with_no_room_for_the_lane(emu_lib):
    n, cols, want = case_row_nearly_full()
    info = check_constructed(emu_lib, n, cols, want, 2, 4, 2)
    # the case is at the boundary only while the rows keep their first stride
    assert info["xcap_digits"] == 16, info["xcap_digits"]
    assert info["max_limbs"] == 8


def test_raw_fill_source_column_longer_than_a_pass(emu_lib):
    n, cols, want = case_long_column()
    check_constructed(emu_lib, n, cols, want, 2, 3, 1)


@pytest.mark.parametrize("waves,workers,seed", [(2, 6, 1), (2, 3, 4)])
def test_raw_fill_through_helpers(emu_farm_lib, waves, workers, seed):
    """the build that opens every queue of two or more items: the raw value travels in the job slot to the helping workgroups"""
    n, cols = base_matrix(-(3 << 5), 0x7FFFFFFF, 0xFEDCBA9876543211)
    info = check_constructed(emu_farm_lib, n, cols, BASE_FILLS, waves, workers, seed)
    assert info["farm_jobs"] > 0


def test_raw_fill_in_weak_store_mode(emu_farm_lib):
    """the same hand-off under delayed, reordered write-through stores"""
    n, cols = base_matrix(-(3 << 5), 0x7FFFFFFF, 0xFEDCBA9876543211)
    check_constructed(emu_farm_lib, n, cols, BASE_FILLS, 2, 6, 11, weak=1)


def test_raw_fill_in_the_forward_solve(emu_lib):
    """the forward substitution is the same sweep: a right-hand side entry above rows that are still zero fills them in;
    numerators against the solve oracle"""
    import slip_lu_amd as sl
    n, cols = base_matrix(-3, 0xF00DF00D, -0x1234567890ABCDEF)
    Ap, Ai, Alen, Alimbs = csc(n, cols)
    q = np.arange(n, dtype=np.int32)
    b = np.zeros(n, np.int64)
    b[1] = -(2 ** 35 + 7); b[6] = 5; b[15] = -3
    _seed(emu_lib, 2)
    f = sl.Factorization(n, Ap, Ai, Alen, Alimbs, q, pivot=DIAGONAL, waves=2, workers=3, lib_path=emu_lib)
    try:
        f.run(0)
        before = f.info()["raw_fills"]
        xlen, xlimbs = f.solve(np.sign(b).astype(np.int32), np.abs(b[b != 0]).astype(np.uint64))
        after = f.info()["raw_fills"]
    finally:
        f.close()
    want, _ = oracle_lib.factorize_and_solve(n, Ap, Ai, Alen, Alimbs, q, b, pivot=DIAGONAL)
    assert oracle_lib.bigints(xlen, xlimbs) == want
    # b[1] is untouched at position 1: it fills the rows of L(:,1) below the diagonal (2..13) but row 6, which holds a value
    assert after - before == 11, (before, after)


@pytest.mark.parametrize("name", sorted(GOLDEN_RUNS))
def test_raw_fill_on_the_goldens(emu_lib, name):
    """the reference's goldens at the (waves, workers) pairs of the committer's tests: same factors, and the path is taken"""
    import slip_lu_amd as sl
    entry, fix = load_case(name)
    for waves, workers, seed, flags in GOLDEN_RUNS[name]:
        _seed(emu_lib, seed)
        res = sl.factorize(entry["n"], fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"], pivot=entry["pivot"], tol=entry["tol"],
                           kmax=entry["kmax"], limb_cap=entry["cap"], waves=waves, workers=workers, lib_path=emu_lib, debug_flags=flags)
        check_against_golden(entry, fix, res)
        info = res["info"]
        assert 0 < info["raw_fills"] <= info["n_upd"], info
