"""Parity of the HIP path (through the C ABI, libslip_hip.so) with the reference.  Bit-exact."""
import os
import random

import numpy as np
import pytest

import oracle_lib
from conftest import check_against_golden, golden_index, load_case

pytestmark = pytest.mark.gpu

ALL = list(golden_index())
HEAVY = {"NSR8K", "fome12", "rail4284", "gen_n2000_pm1"}


def _run(entry, fix, **kw):
    import slip_lu_amd as sl
    return sl.factorize(entry["n"], fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"],
                        pivot=entry["pivot"], tol=entry["tol"], kmax=entry["kmax"], limb_cap=entry["cap"],
                        check=False, **kw)


@pytest.mark.parametrize("name", [n for n in ALL if n not in HEAVY])
def test_gpu_matches_reference_golden(name):
    entry, fix = load_case(name)
    res = _run(entry, fix)
    assert res["status"] == entry["status"]
    check_against_golden(entry, fix, res)


@pytest.mark.parametrize("name", sorted(HEAVY))
def test_gpu_matches_reference_golden_heavy(name):
    entry, fix = load_case(name)
    res = _run(entry, fix)
    assert res["status"] == entry["status"]
    check_against_golden(entry, fix, res)


@pytest.mark.parametrize("waves", [1, 2, 4, 8])
def test_gpu_wave_count_independent(waves):
    entry, fix = load_case("prob159")
    check_against_golden(entry, fix, _run(entry, fix, waves=waves))


def test_gpu_matches_oracle_on_fresh_seeds():
    """Seeded synthetic inputs that have no golden: HIP path vs the CPU restatement, same run."""
    import slip_lu_amd as sl
    # (n, density, bits, kmax): sized so the CPU restatement finishes in seconds (values reach ~170 limbs)
    for seed, (n, d, b, kmax) in enumerate([(60, 0.1, 16, 0), (200, 0.03, 40, 0), (500, 0.01, 3, 0),
                                            (1500, 0.002, 16, 800)], start=11):
        Ap, Ai, Ax = oracle_lib.matgen(n, d, b, seed)
        Alen, Alimbs = np.sign(Ax).astype(np.int32), np.abs(Ax).astype(np.uint64)
        q = np.random.RandomState(seed).permutation(n).astype(np.int32)
        for pivot in (3, 0, 5, 1, 2, 4) if n < 1000 else (3,):
            tol = 0.5 if pivot == 4 else 1.0
            ref = oracle_lib.factorize(n, Ap, Ai, Alen, Alimbs, q, pivot=pivot, tol=tol, kmax=kmax)
            got = sl.factorize(n, Ap, Ai, Alen, Alimbs, q, pivot=pivot, tol=tol, kmax=kmax, check=False)
            assert got["status"] == ref["status"] and got["K"] == ref["K"]
            for k in ("pinv", "Lp", "Li", "Llen", "Llimbs", "Up", "Ui", "Ulen", "Ulimbs", "rholen", "rholimbs"):
                assert np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(ref[k]).astype(np.int64)), (seed, pivot, k)
            assert list(got["counters"][:6]) == list(ref["counters"][:6])
            assert int(got["counters"][7]) == int(ref["counters"][7])          # limb-MAC counter


def test_gpu_multilimb_inputs_and_duplicates():
    """A with multi-limb entries, unsorted rows and a duplicated (row, col): the last value wins
    (slip_get_column.c:22)."""
    import slip_lu_amd as sl
    rnd = random.Random(5)
    n = 12
    cols, Ap = [], [0]
    for j in range(n):
        rows = rnd.sample(range(n), 4)
        if j not in rows:
            rows[0] = j
        rows.append(rows[1])                       # duplicate
        cols.append(rows)
        Ap.append(Ap[-1] + len(rows))
    Ai = np.array([r for c in cols for r in c], dtype=np.int32)
    lens, limbs = [], []
    for _ in range(len(Ai)):
        l = rnd.choice([1, 1, 2, 3])
        v = [rnd.getrandbits(64) | 1 for _ in range(l)]
        lens.append(l if rnd.random() < 0.5 else -l)
        limbs += v
    Ap = np.array(Ap, dtype=np.int64)
    Alen, Alimbs = np.array(lens, dtype=np.int32), np.array(limbs, dtype=np.uint64)
    q = np.arange(n, dtype=np.int32)[::-1].copy()
    ref = oracle_lib.factorize(n, Ap, Ai, Alen, Alimbs, q)
    got = sl.factorize(n, Ap, Ai, Alen, Alimbs, q, check=False)
    assert got["status"] == ref["status"] == 0
    for k in ("pinv", "Li", "Llen", "Llimbs", "Ui", "Ulen", "Ulimbs", "rholimbs"):
        assert np.array_equal(got[k], ref[k]), k


def test_gpu_singular_and_bad_input():
    import slip_lu_amd as sl
    Ap = np.array([0, 2, 4, 5], dtype=np.int64)
    Ai = np.array([0, 1, 0, 1, 0], dtype=np.int32)
    Ax = np.array([2, 3, 5, 7, 11], dtype=np.int64)
    got = sl.factorize(3, Ap, Ai, np.sign(Ax).astype(np.int32), np.abs(Ax).astype(np.uint64),
                       np.arange(3, dtype=np.int32), check=False)
    assert got["status"] == -2 and got["K"] == 2           # SLIP_SINGULAR at column 2
    with pytest.raises(sl.SlipError) as e:                  # row index out of range
        sl.factorize(3, Ap, np.array([0, 1, 0, 9, 0], dtype=np.int32), np.ones(5, np.int32),
                     np.ones(5, np.uint64), np.arange(3, dtype=np.int32))
    assert e.value.code == -3


def test_gpu_reset_is_idempotent_and_resumable():
    """reset + rerun gives the same bytes; running [0,K1) then [K1,n) equals one run."""
    import slip_lu_amd as sl
    import slabfile
    entry, fix = load_case("prob159")
    f = sl.Factorization(entry["n"], fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"])
    f.run()
    d1 = slabfile.factor_digest(f.download())
    f.reset(); f.run(300); f.run()
    d2 = slabfile.factor_digest(f.download())
    f.close()
    assert d1 == d2 == entry["digest"]


def _digits(v, n):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


@pytest.mark.parametrize("op", [0, 1, 2, 3, 10, 11, 12, 13])
def test_gpu_wave_limb_ops(op):
    """wave_bigint.h / wave_bigint_reg.h primitives on the device vs Python integers."""
    import ctypes as C
    from slip_lu_amd import _lib
    lib = _lib.load()
    rnd = random.Random(100 + op)
    for la, lb, W in [(1, 1, 2), (2, 5, 7), (64, 64, 128), (65, 3, 66), (130, 129, 200), (100, 128, 64), (7, 200, 207),
                      (128, 128, 256), (200, 256, 256)]:
        if op >= 10 and W > 256:
            continue
        nops = 24
        A, B, exp = [], [], []
        for t in range(nops):
            kind = t % 4
            a = rnd.getrandbits(32 * la) if kind else (1 << (32 * la)) - 1
            b = rnd.getrandbits(32 * lb) if kind != 1 else (1 << (32 * lb)) - 1
            if op % 10 == 3:
                a |= 1
            A += _digits(a, la); B += _digits(b, lb)
            m = 1 << (32 * W)
            if op % 10 == 0: e = (a * b) % m
            elif op % 10 == 1: e = (a % m + b % m) % m
            elif op % 10 == 2: e = (a % m - b % m) % m
            else: e = pow(a, -1, m)
            exp += _digits(e, W)
        a_ = np.array(A, dtype=np.uint32); b_ = np.array(B, dtype=np.uint32); out = np.zeros(nops * W, dtype=np.uint32)
        rc = lib.slip_hip_wave_op_test(op, nops, la, lb, W, a_.ctypes.data, b_.ctypes.data, out.ctypes.data)
        assert rc == 0
        assert np.array_equal(out, np.array(exp, dtype=np.uint32)), (op, la, lb, W)


def _hensel_cases(lib):
    """exact division without an inverse (wr_div_hensel, wave_bigint_reg.h) vs Python integers: T = q * d mod B^W -> q;
    (W, digits of d) as VERDICT r2 item 3 names them plus the edges (one digit, chunk borders, all-ones operands)"""
    import ctypes as C
    lib.slip_hip_wave_op_test.argtypes = [C.c_int32] * 5 + [C.c_void_p] * 3
    rnd = random.Random(715)
    for W, ld in [(1, 1), (2, 1), (5, 3), (16, 8), (64, 64), (65, 2), (128, 64), (130, 129), (200, 128), (256, 256), (256, 1), (63, 64), (192, 100)]:
        nops = 12
        A, B, exp = [], [], []
        for t in range(nops):
            q = rnd.getrandbits(32 * W) if t % 3 else (1 << (32 * W)) - 1
            d = rnd.getrandbits(32 * ld) | 1
            if t == 2: d = (1 << (32 * ld)) - 1
            if t == 5: q = 0
            if t == 7: d = 1
            m = 1 << (32 * W)
            A += _digits((q * d) % m, W); B += _digits(d, ld); exp += _digits(q % m, W)
        a_ = np.array(A, dtype=np.uint32); b_ = np.array(B, dtype=np.uint32); out = np.zeros(nops * W, dtype=np.uint32)
        assert lib.slip_hip_wave_op_test(15, nops, W, ld, W, a_.ctypes.data, b_.ctypes.data, out.ctypes.data) == 0
        assert np.array_equal(out, np.array(exp, dtype=np.uint32)), (W, ld)


def test_gpu_wave_hensel_division():
    from slip_lu_amd import _lib
    _hensel_cases(_lib.load())


def test_gpu_wave_reductions():
    """the DPP wave reductions / lane-0 broadcast of wave_shim.h (used on the commit chain) vs numpy"""
    from slip_lu_amd import _lib
    lib = _lib.load()
    rnd = np.random.RandomState(3)
    nops = 16
    a = rnd.randint(0, 2 ** 24, size=nops * 64).astype(np.uint32)
    a[64:128] = 0; a[128:192] = 0xFFFFFFFF >> 8; a[192] = 7
    b = np.zeros(nops, np.uint32)
    for op, fn in ((24, lambda v: np.uint32(v.sum() & 0xFFFFFFFF)), (25, lambda v: v.max()), (26, lambda v: v.min()), (27, lambda v: v[0])):
        out = np.zeros(nops * 64, np.uint32)
        assert lib.slip_hip_wave_op_test(op, nops, 64, 1, 64, a.ctypes.data, b.ctypes.data, out.ctypes.data) == 0
        for t in range(nops):
            assert (out[64 * t:64 * t + 64] == fn(a[64 * t:64 * t + 64])).all(), (op, t)


def test_gpu_farm_device_path():
    """SURVEY 8(e) end to end on the device: blocks factorised by the HIP path, pivot chains exchanged (world 1 here),
    columns rescaled by slip_hip_factor_rescale, equal to the HIP factorisation of the whole matrix"""
    import slip_lu_amd as sl
    import test_subtree_farm as T

    def whole(n, Ap, Ai, Ax, q):
        Alen, Alimbs = sl.ints_to_slab(Ax)
        return sl.factorize(n, Ap, Ai, Alen, Alimbs, q)
    T.farm_vs_whole(whole, None)
    T.farm_vs_whole(whole, None, sizes=(40, 25, 60, 33), seed=5)


@pytest.mark.parametrize("name", ["gen_n40", "prob159", "gen_n300"])
def test_gpu_rescale_kernel(name):
    """the farm's device rescale (one wavefront per stored entry; products up to several hundred digits)"""
    from test_emu_kernel import check_rescale
    check_rescale(None, name, 11)


def test_gpu_subtree_farm_law():
    """independent diagonal blocks factorised one by one on the HIP path and reassembled with
    slip_lu_amd.parallel (pivot chains -> scales) equal the HIP factorisation of the whole matrix."""
    import slip_lu_amd as sl
    import test_subtree_farm as T

    def gpu_factor(n, Ap, Ai, Ax, q):
        Alen, Alimbs = sl.ints_to_slab(Ax)
        r = sl.factorize(n, Ap, Ai, Alen, Alimbs, q)
        assert r["status"] == 0 and r["K"] == n
        return r
    T.check_farm(gpu_factor)
    T.check_farm(gpu_factor, sizes=(40, 25, 60), seed=5)


@pytest.mark.parametrize("name,kw", [("prob159", dict(workers=1)), ("prob159", dict(workers=2, waves=1)), ("gen_n300", dict(workers=7, waves=2)),
                                     ("rl5934", dict(workers=64)), ("rl5934", dict(workers=4096, waves=8)),
                                     ("C4_n100k_c64", dict(workers=3)), ("C4_n100k_c64", dict(workers=1000)),
                                     ("NSR8K_w600", dict(workers=2048, waves=2)), ("10teams", dict(workers=177))])
def test_gpu_worker_count_independent(name, kw):
    """Every column goes through the worker pipeline; the factors must not depend on how many workers run ahead of
    the commit frontier -- one worker (no look-ahead at all), a handful, one per column, or far more workgroups than
    the device can hold at once (a workgroup that is not resident holds no column ticket, so nothing waits for it)."""
    entry, fix = load_case(name)
    res = _run(entry, fix, **kw)
    assert res["status"] == entry["status"]
    check_against_golden(entry, fix, res)


def test_gpu_tied_pivots_under_load():
    """fome12 has columns whose best pivot candidates tie in magnitude over several limbs: the exact comparison of the early
    commit runs while other waves are busy (a race here once published one row and copied the other); ten runs, two shapes"""
    import slip_lu_amd as sl
    import slabfile
    entry, fix = load_case("fome12")
    for workers in (32, 0):
        f = sl.Factorization(entry["n"], fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"], workers=workers)
        try:
            for rep in range(5):
                f.reset(); f.run()
                got = f.download()
                assert np.array_equal(got["pinv"], fix["pinv"]) and slabfile.factor_digest(got) == entry["digest"], (workers, rep)
        finally:
            f.close()


def test_gpu_limb_mac_counter_matches_oracle():
    """the ALU-roofline counter, sum over the IPGE updates of l(L_m) l(x_j) + l(x_i) l(rho_jn) in 64-bit
    limbs, counted by the device == the CPU restatement's ORC_LIMB_MACS (12 440 261 on the headline window)."""
    entry, fix = load_case("C4_n100k_c64")
    res = _run(entry, fix)
    assert res["info"]["limb_macs"] == 12440261
    for name in ("prob159", "10teams", "gen_n300"):
        entry, fix = load_case(name)
        res = _run(entry, fix)
        ref = oracle_lib.factorize(entry["n"], fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"],
                                   pivot=entry["pivot"], kmax=entry["kmax"])
        assert res["info"]["limb_macs"] == int(ref["counters"][7]), name


def test_gpu_repeated_runs_under_load_are_identical():
    """The hand-offs between workers (commit frontier, ready frontier, inverse cache) under uneven load: the same
    factorisation twenty times on a handle, different worker counts interleaved, always the reference's bytes."""
    import slip_lu_amd as sl
    import slabfile
    entry, fix = load_case("rl5934")
    handles = [sl.Factorization(entry["n"], fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"], workers=w, waves=wv)
               for w, wv in ((0, 0), (5, 2), (97, 1))]
    try:
        for rep in range(7):
            for f in handles:
                f.reset(); f.run()
                assert slabfile.factor_digest(f.download()) == entry["digest"], rep
    finally:
        for f in handles:
            f.close()


@pytest.mark.gpu
def test_gpu_triplet_file_to_factors():
    """a Demo/SLIPLU.c-shaped path without the reference's reader: the triplet file goes through slip_hip_read_triplet into
    limb slabs, through the factorisation, and the factors equal the reference's golden record"""
    import os
    import slip_lu_amd as sl
    from conftest import GOLDEN
    entry, fix = load_case("test_mat")
    n, Ap, Ai, Alen, Al = sl.read_triplet(os.path.join(GOLDEN, "test_mat_triplet.txt"))
    res = sl.factorize(n, Ap, Ai, Alen, Al, fix["q"], pivot=entry["pivot"], tol=entry["tol"], kmax=entry["kmax"], limb_cap=entry["cap"])
    check_against_golden(entry, fix, res)


@pytest.mark.gpu
def test_gpu_verdicts_survive_slot_reuse():
    """two-wave workers are slow to read their verdict: the package slot of column k is reused by column k + workers
    before that (the verdict lives in the WORKER's mailbox, not in the slot).  Repeated on one handle: every run must
    end with the reference's factors (a lost verdict used to end in a 20 s spin-limit abort every ~25th run)."""
    import slip_lu_amd as sl
    import slabfile
    entry, fix = load_case("C4_n100k_c64")
    f = sl.Factorization(entry["n"], fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"], pivot=entry["pivot"], tol=entry["tol"],
                         limb_cap=entry["cap"], waves=2)
    try:
        for rep in range(60):
            f.reset()
            rc = f.run(entry["kmax"], check=False)
            i = f.info()
            assert rc == 0 and i["K"] == entry["K"], (rep, rc, i["K"])
            assert i["committer_commits"] > 0
        d = f.download()
        assert np.array_equal(d["pinv"], fix["pinv"]) and slabfile.factor_digest(d) == entry["digest"]
    finally:
        f.close()
