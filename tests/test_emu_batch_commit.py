"""The committer's run (ref_lu_pipe_commit.h, slip_commit_run_out): the candidates-only columns of a batch whose pivots the
load step has chosen are committed side by side, the rest of the batch by the serial step.  On the CPU emulation of the
kernel source, bit-exact against the reference's goldens or the CPU restatement (oracle_lib.factorize)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
from conftest import ROOT, check_against_golden, load_case

EMU = os.path.join(ROOT, "tests", "emu", "libslip_emu.so")
FACTOR_KEYS = ("pinv", "Lp", "Li", "Llen", "Llimbs", "Up", "Ui", "Ulen", "Ulimbs", "rholen", "rholimbs")


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "libslip_emu.so"])
    return EMU


def _lib(path, seed, weak=0):
    lib = ctypes.CDLL(path)
    lib.slip_emu_set_seed.argtypes = [ctypes.c_ulonglong]
    lib.slip_emu_set_seed(seed)
    lib.slip_emu_set_weak(weak)
    return lib


def _golden_run(emu_lib, name, waves, workers, seed, weak=0, **kw):
    import slip_lu_amd as sl
    entry, fix = load_case(name)
    lib = _lib(emu_lib, seed, weak)
    try:
        res = sl.factorize(entry["n"], fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"], pivot=entry["pivot"], tol=entry["tol"],
                           kmax=entry["kmax"], limb_cap=entry["cap"], waves=waves, workers=workers, lib_path=emu_lib, **kw)
    finally:
        lib.slip_emu_set_weak(0)
    check_against_golden(entry, fix, res)
    return res["info"]


# (waves, workers, seed, debug flags): eight emulated waves cost many times two, so they run on the smallest golden only
GOLDEN_RUNS = {"gen_n40": ((1, 6, 1, 0), (2, 9, 2, 8)), "gen_n40_pm1": ((2, 24, 4, 8),), "test_mat": ((8, 5, 3, 0), (1, 4, 2, 8)),
               "10teams": ((2, 9, 2, 0),)}


@pytest.mark.parametrize("name", sorted(GOLDEN_RUNS))
def test_emulated_run_matches_reference(emu_lib, name):
    """goldens with candidates-only commits at one, two and eight waves and several worker counts, the chain engine on and off
    (on these small dense matrices a batch seldom starts with two such columns: the constructed cases below make runs)"""
    for waves, workers, seed, flags in GOLDEN_RUNS[name]:
        info = _golden_run(emu_lib, name, waves, workers, seed, debug_flags=flags)
        assert info["batch_commits"] <= info["committer_commits"] - info["engine_commits"], info


@pytest.mark.parametrize("name,workers,waves,seed", [("10teams", 9, 2, 11), ("gen_n40_pm1", 24, 1, 5)])
def test_emulated_run_in_weak_store_mode(emu_lib, name, workers, waves, seed):
    """the run's permutation stores under delayed, reordered write-through stores"""
    _golden_run(emu_lib, name, waves, workers, seed, weak=1, check=False)


def _csc(n, cols):
    """cols: {column: {row: value}} -> (Ap, Ai, Alen, Alimbs)"""
    Ap, Ai, vals = [0], [], []
    for j in range(n):
        for i in sorted(cols.get(j, {})):
            Ai.append(i)
            vals.append(cols[j][i])
        Ap.append(len(Ai))
    v = np.array(vals, dtype=np.int64)
    return (np.array(Ap, dtype=np.int64), np.array(Ai, dtype=np.int32), np.sign(v).astype(np.int32),
            np.abs(v).astype(np.uint64))


def _check_constructed(emu_lib, n, cols, pivot, waves, workers, seed, **kw):
    import slip_lu_amd as sl
    Ap, Ai, Alen, Alimbs = _csc(n, cols)
    q = np.arange(n, dtype=np.int32)
    _lib(emu_lib, seed)
    got = sl.factorize(n, Ap, Ai, Alen, Alimbs, q, pivot=pivot, waves=waves, workers=workers, lib_path=emu_lib, check=False, **kw)
    ref = oracle_lib.factorize(n, Ap, Ai, Alen, Alimbs, q, pivot=pivot)
    assert got["K"] == ref["K"], (got["K"], ref["K"])
    for k in FACTOR_KEYS:
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(ref[k]).astype(np.int64)), k
    return got["info"]


def _diagonal(n, rng):
    return {j: {j: int(rng.randint(200, 900)) * (1 if rng.rand() < 0.7 else -1)} for j in range(n)}


def test_emulated_run_claim_conflict(emu_lib):
    """consecutive columns whose sole smallest candidate is the same row: the second one's package goes back inside the
    batch (its pattern holds the row the first one has just made pivotal) and still comes out right"""
    rng = np.random.RandomState(7)
    n = 32
    total = 0
    for rep, (waves, workers, seed) in enumerate(((2, 12, 1), (1, 8, 4), (8, 6, 7))):
        cols = _diagonal(n, rng)
        shared = n - 1 - rep
        for j in range(4, 20, 3):
            cols[j][shared] = 3 + rep
            cols[j + 1][shared] = 5 + rep
        total += _check_constructed(emu_lib, n, cols, 0, waves, workers, seed)["batch_commits"]
    assert total > 0


def test_emulated_run_tie_in_the_middle(emu_lib):
    """a column with two equal smallest candidates in the middle of candidates-only columns: the run ends before it and the
    serial step breaks the tie by positions"""
    rng = np.random.RandomState(3)
    n = 32
    total = 0
    for rep, (waves, workers, seed) in enumerate(((2, 12, 1), (1, 10, 5))):
        cols = _diagonal(n, rng)
        for j in range(6, n - 10, 5):
            cols[j][j + 7] = 11 + rep
            cols[j][j + 9] = -(11 + rep)
        total += _check_constructed(emu_lib, n, cols, 0, waves, workers, seed)["batch_commits"]
    assert total > 0


def test_emulated_run_capacity_reject(emu_lib):
    """slabs sized far too small: a capacity check fails, the serial step rejects that column, the slabs grow and the launch
    goes on"""
    _golden_run(emu_lib, "gen_n40_pm1", 2, 6, 2, lnz_hint=1, unz_hint=1)


def test_emulated_run_capacity_reject_constructed(emu_lib):
    """the same on a matrix whose batches are runs of candidates-only columns: the first column that does not fit ends the run"""
    rng = np.random.RandomState(5)
    n = 32
    cols = _diagonal(n, rng)
    for j in range(3, n - 6, 4):
        cols[j][j + 5] = int(rng.randint(1, 9))
    assert _check_constructed(emu_lib, n, cols, 0, 2, 12, 1, lnz_hint=1, unz_hint=1)["batch_commits"] > 0
