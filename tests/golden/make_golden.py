#!/usr/bin/env python3
"""Generate the golden fixtures under tests/golden/ from the COMPILED REFERENCE.

Runs only where /root/reference exists (this container): it executes
oracle/_ref/ref_driver, which oracle/Makefile builds from the unmodified
reference sources, and records for every case

  * the input as data: the CSC arrays of the reference's own example matrices
    (SLIP_LU/ExampleMats, data files its demos/tests hold) or the spec of the
    deterministic generator (slip_matgen.h),
  * the column order q the reference's SLIP_LU_analyze (COLAMD/AMD/none) chose,
  * the reference's result: full L/U/rho/pinv arrays for small cases, a SHA-256
    over the canonical arrays for large ones, plus the algorithmic counters of
    SURVEY.md 8(d) and the reference's own wall time.

Nothing of the reference's source travels; fixtures are inputs and outputs.
Usage:  python tests/golden/make_golden.py [case ...]
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import slabfile  # noqa: E402

REF = "/root/reference/SLIP_LU/ExampleMats"
DRIVER = os.path.join(ROOT, "oracle", "_ref", "ref_driver")

# name: (input spec, pivot, order, tol, K, cap, keep_full_factor)
CASES = {
    # the reference's own example matrices, default options (COLAMD, TOL_SMALLEST, tol 1)
    "test_mat":        (f"trip:{REF}/test_mat.txt", 3, 1, 1.0, 0, 0, True),
    "10teams":         (f"trip:{REF}/10teams_mat.txt", 3, 1, 1.0, 0, 0, False),
    "prob159":         (f"trip:{REF}/prob159_mat.txt", 3, 1, 1.0, 0, 0, False),
    "NSR8K":           (f"trip:{REF}/NSR8K_mat.txt", 3, 1, 1.0, 0, 0, False),
    "NSR8K_w600":      (f"trip:{REF}/NSR8K_mat.txt", 3, 1, 1.0, 600, 0, False),
    # every pivoting scheme and ordering on small inputs
    "test_mat_p0":     (f"trip:{REF}/test_mat.txt", 0, 1, 1.0, 0, 0, True),
    "test_mat_p1":     (f"trip:{REF}/test_mat.txt", 1, 1, 1.0, 0, 0, True),
    "test_mat_p2":     (f"trip:{REF}/test_mat.txt", 2, 1, 1.0, 0, 0, True),
    "test_mat_p4":     (f"trip:{REF}/test_mat.txt", 4, 1, 1.0, 0, 0, True),
    "test_mat_p5":     (f"trip:{REF}/test_mat.txt", 5, 1, 1.0, 0, 0, True),
    "test_mat_noord":  (f"trip:{REF}/test_mat.txt", 3, 0, 1.0, 0, 0, True),
    "test_mat_amd":    (f"trip:{REF}/test_mat.txt", 3, 2, 1.0, 0, 0, True),
    "test_mat_tol01":  (f"trip:{REF}/test_mat.txt", 3, 1, 0.1, 0, 0, True),
    "test_mat_p4tol":  (f"trip:{REF}/test_mat.txt", 4, 1, 0.3, 0, 0, True),
    "10teams_p0":      (f"trip:{REF}/10teams_mat.txt", 0, 1, 1.0, 0, 0, False),
    "10teams_p5":      (f"trip:{REF}/10teams_mat.txt", 5, 1, 1.0, 0, 0, False),
    "10teams_tol":     (f"trip:{REF}/10teams_mat.txt", 3, 1, 0.01, 0, 0, False),
    "prob159_p1":      (f"trip:{REF}/prob159_mat.txt", 1, 1, 1.0, 0, 0, False),
    "prob159_p4tol":   (f"trip:{REF}/prob159_mat.txt", 4, 1, 0.5, 0, 0, False),
    "prob159_w200c8":  (f"trip:{REF}/prob159_mat.txt", 3, 1, 1.0, 0, 8, False),
    # LP bases shipped with the reference (complete runs spanning the limb classes)
    "rail4284":        (f"trip:{REF}/BasisLIB_ALL/RHS/rail4284.mat", 3, 1, 1.0, 0, 0, False),
    "fome12":          (f"trip:{REF}/BasisLIB_ALL/RHS/fome12.mat", 3, 1, 1.0, 0, 0, False),
    "rl5934":          (f"trip:{REF}/BasisLIB_ALL/RHS/rl5934.mat", 3, 1, 1.0, 0, 0, False),
    "d18512":          (f"trip:{REF}/BasisLIB_ALL/RHS/d18512.mat", 3, 1, 1.0, 0, 0, False),
    "model6":          (f"trip:{REF}/BasisLIB_ALL/RHS/model6.mat", 3, 1, 1.0, 0, 0, False),
    "de080285":        (f"trip:{REF}/BasisLIB_ALL/RHS/de080285.mat", 3, 1, 1.0, 0, 0, False),
    # synthetic matrices of the benchmark shapes (generator spec: n,density,bits,seed)
    "gen_n40":         ("gen:40,0.15,8,5", 3, 1, 1.0, 0, 0, True),
    "gen_n40_pm1":     ("gen:40,0.2,1,6", 3, 1, 1.0, 0, 0, True),
    "gen_n300":        ("gen:300,0.01,16,2", 3, 1, 1.0, 0, 0, False),
    "gen_n2000_pm1":   ("gen:2000,0.002,1,7", 3, 1, 1.0, 0, 0, False),
    "gen_n5000_c8":    ("gen:5000,0.0008,16,3", 3, 1, 1.0, 0, 8, False),
    "gen_n20000_c16":  ("gen:20000,0.001,16,1", 3, 1, 1.0, 0, 16, False),
    "C3_n50k_c32":     ("gen:50000,0.001,16,1", 3, 1, 1.0, 0, 32, False),
    "C4_n100k_c64":    ("gen:100000,0.001,16,1", 3, 1, 1.0, 0, 64, False),
    "C5_n200k_c64":    ("gen:200000,0.0005,16,1", 3, 1, 1.0, 0, 64, False),
}


def run_case(name):
    spec, pivot, order, tol, K, cap, full = CASES[name]
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "o.slab")
        subprocess.check_call([DRIVER, "window", spec, out, str(K), str(cap), str(pivot), str(order), repr(tol)])
        d = slabfile.load(out)
        entry = dict(name=name, input=spec if spec.startswith("gen:") else "slab", pivot=pivot, order=order,
                     tol=tol, kmax=K, cap=cap, n=int(d["n"][0]), K=int(d["K"][0]),
                     status=int(d["counters"][7]),
                     lnz=int(len(d.get("Li", []))), unz=int(len(d.get("Ui", []))),
                     counters={k: int(v) for k, v in zip(
                         ("N_upd", "B_read", "B_write", "N_src", "L_streamed", "maxlimbs", "K_done"), d["counters"][:7])},
                     ref_seconds=float(d["timing"][0]), ref_sym_seconds=float(d["timing"][1]),
                     digest=slabfile.factor_digest(d) if int(d["K"][0]) > 0 else None, full=full)
        fix = {"q": d["q"], "pinv": d["pinv"]}
        if not spec.startswith("gen:"):
            subprocess.check_call([DRIVER, "order", spec, os.path.join(td, "a.slab"), str(order)],
                                  stderr=subprocess.DEVNULL)
            a = slabfile.load(os.path.join(td, "a.slab"))
            assert np.array_equal(a["q"], d["q"])
            for k in ("Ap", "Ai", "Alen", "Alimbs"):
                fix[k] = a[k]
        if full:
            for k in slabfile.FACTOR_KEYS:
                fix[k] = d[k]
        else:
            fix["rholen"] = d["rholen"]
        slabfile.save(os.path.join(HERE, name + ".slab.gz"), fix)
        return entry


# rational solutions of SLIP_LU_solve for the deterministic right-hand side of ref_driver's `solve` mode
SOLVE_CASES = {
    "solve_test_mat": f"trip:{REF}/test_mat.txt",
    "solve_10teams":  f"trip:{REF}/10teams_mat.txt",
    "solve_gen_n40":  "gen:40,0.15,8,5",
}


def run_solve_cases():
    idx = []
    with tempfile.TemporaryDirectory() as td:
        for name, spec in SOLVE_CASES.items():
            out = os.path.join(td, "s.slab")
            subprocess.check_call([DRIVER, "solve", spec, out], stderr=subprocess.DEVNULL)
            d = slabfile.load(out)
            fix = {k: d[k] for k in ("q", "pinv", "xnumlen", "xnumlimbs", "xdenlen", "xdenlimbs")}
            if not spec.startswith("gen:"):
                subprocess.check_call([DRIVER, "order", spec, os.path.join(td, "a.slab")], stderr=subprocess.DEVNULL)
                a = slabfile.load(os.path.join(td, "a.slab"))
                for k in ("Ap", "Ai", "Alen", "Alimbs"):
                    fix[k] = a[k]
            slabfile.save(os.path.join(HERE, name + ".slab.gz"), fix)
            idx.append(dict(name=name, input=spec if spec.startswith("gen:") else "slab", n=int(d["n"][0])))
    json.dump(idx, open(os.path.join(HERE, "solve_index.json"), "w"), indent=1)


# ---- the pivot-edge corpus (pivot_corpus.json + pivot_corpus.slab.gz) ----
# Small signed matrices whose columns put the candidates of slip_get_pivot in the places where a pivot rule can be
# read wrongly: a negative largest candidate (scheme 4), magnitude ties with opposite signs, multi-limb candidates that
# tie on the kernel's search key (bit length, top 40 bits) or are equal over several limbs, tolerance ratios exactly
# on tol and one unit below it, a diagonal that is an explicit zero / missing / already pivotal, explicit zeros
# first in the pattern, a singular column.  Crafted columns sit at the first column of a block of a block
# lower-triangular matrix: there the block's rows are untouched, so a candidate is a*rho[k-1] and the crafted ties,
# ratios and signs survive into multi-limb values (both sign polarities of a block are emitted, as the sign of
# rho[k-1] is whatever the preceding blocks made it).  Column order 0: a crafted column stays where it was placed.
# Every matrix runs under every scheme; schemes 3 and 4 under each tolerance of CORPUS_TOLS (0.375: the exact-tie
# value the crafted 3:8 ratios hit).  Deterministic: the same seed gives the same bytes (gzip mtime 0).
CORPUS_SEED = 20261015
CORPUS_TOLS = (1.0, 0.5, 0.3, 0.1, 2.0 ** -20, 0.375)
# candidate sizes: one limb (the in-lane paths), a few limbs, and register sizes up to and beyond the D=4 cap of
# 256 32-bit digits (8192 bits)
CORPUS_BITS = (20, 62, 64, 130, 1500, 8150, 8300)
RATIO_BITS = (20, 64, 130, 8150)


def _corpus_blocks(rnd):
    """[(label, first-column entries {block row: value}, block size)] -- rows relative to the block, row 0 is the diagonal
    (absent from the dict: no entry; 0: an explicit zero)."""
    B = []

    def big(bits):
        return (1 << (bits - 1)) | rnd.getrandbits(bits - 1)

    for bits in CORPUS_BITS:
        v = big(bits)
        # the largest candidate negative, the diagonal smaller / equal / an explicit zero / missing
        B.append(("neg_largest_diag_smaller", {0: v // 3 + 1, 1: -v, 2: v // 2}, 4))
        B.append(("neg_largest_diag_equal", {0: v, 1: -v, 2: v // 5}, 4))
        B.append(("neg_largest_diag_zero", {0: 0, 1: -v, 2: v // 7}, 4))
        B.append(("neg_largest_diag_missing", {1: v // 9, 2: -v}, 3))
        # equal magnitudes, opposite signs: position order decides (schemes 0, 3, 4, 5)
        B.append(("signed_tie_large", {0: v // 11 + 1, 1: v, 2: -v, 3: -v}, 4))
        B.append(("signed_tie_small", {0: v, 1: -(v // 13 + 1), 2: v // 13 + 1, 3: v // 2}, 4))
        # equal bit length and top 40 bits, differing lower down; equal over several limbs
        if bits > 48:
            d = rnd.randrange(1, 1 << 12)
            B.append(("key_tie_low_digits", {0: v >> 3, 1: v, 2: -(v + d), 3: v + d - 1}, 4))
            B.append(("key_tie_low_digits_small", {0: v, 1: -(v >> 4) - d, 2: (v >> 4) + d - 1, 3: -((v >> 4) + d)}, 4))
        # ratios exactly on a dyadic tol, and one unit below it (scheme 4: |diag|/|largest|; scheme 3: |smallest|/|diag|)
        for num, den in (((1, 2), (3, 8), (1, 1 << 20), (3, 10), (1, 1)) if bits in RATIO_BITS else ()):
            w = v >> 21 if bits > 40 else v
            B.append((f"ratio_{num}_{den}", {0: num * w, 1: den * w, 2: -(num * w - 1) if num * w > 1 else 7}, 3))
            B.append((f"ratio_{num}_{den}_below", {0: num * w - 1 if num * w > 1 else 1, 1: -den * w, 2: den * w - 1}, 3))
            B.append((f"ratio3_{num}_{den}", {0: den * w, 1: num * w, 2: -(den * w + 1)}, 3))
            B.append((f"ratio3_{num}_{den}_below", {0: -den * w, 1: num * w - 1 if num * w > 1 else 1, 2: den * w + 2}, 3))
        # 1/10 with tol 0.1: the double 0.1 is above 1/10, the diagonal is not taken
        w = v >> 4 if bits > 8 else v
        B.append(("ratio_1_10", {0: w, 1: 10 * w, 2: 3 * w}, 3))
        B.append(("ratio3_1_10", {0: 10 * w, 1: -w, 2: 3 * w}, 3))
        # explicit zeros first in the pattern (scheme 2), the diagonal among them
        B.append(("zeros_first", {0: 0, 1: 0, 2: -v, 3: v // 3}, 4))
    return B


def _corpus_matrix(rnd, blocks, singular=False):
    """a block lower-triangular matrix: each block's first column as crafted, its other columns small random values,
    a few couplings into later blocks' rows (after the block's first column, so crafted columns stay clean)"""
    n = sum(m for _, _, m in blocks)
    ent = {}
    s = 0
    starts = []
    for bi, (_, col0, m) in enumerate(blocks):
        starts.append(s)
        for r, v in col0.items():
            ent[(s + r, s)] = v
        for j in range(1, m):
            for r in range(m):
                if r == 0 and j == 1 and 0 not in col0 and bi % 2 == 0:
                    continue       # the diagonal row of column s is the only source of row s: keep a missing diagonal missing
                ent[(s + r, s + j)] = rnd.choice([1, -1]) * rnd.randrange(1, 1 << rnd.choice([3, 20, 63, 64, 100]))
        s += m
    # couplings: column c of a block into a row of a later block (never a later block's first column)
    for bi in range(len(blocks) - 1):
        for _ in range(2):
            c = starts[bi] + rnd.randrange(1, blocks[bi][2])
            r = starts[bi + 1] + rnd.randrange(blocks[bi + 1][2])
            ent[(r, c)] = rnd.choice([1, -1]) * rnd.randrange(1, 1 << 40)
    if singular:
        # the last column a copy of the one before it: no eligible candidate once that one is committed
        for key in [key for key in ent if key[1] == n - 1]:
            del ent[key]
        for (r, c), v in list(ent.items()):
            if c == n - 2:
                ent[(r, n - 1)] = v
    return n, ent


def _corpus_random(rnd):
    """a small random signed matrix with many ties: values drawn from a pool of +-v, v from 1 up to 2^200"""
    n = rnd.randint(2, 9)
    pool = [rnd.choice([1, 2, 3, rnd.getrandbits(rnd.choice([8, 64, 65, 130, 200])) | 1]) for _ in range(rnd.randint(1, 4))]
    dens = rnd.choice([0.4, 0.6, 0.9])
    ent = {}
    for j in range(n):
        for i in range(n):
            if i == j or rnd.random() < dens:
                ent[(i, j)] = rnd.choice([1, -1]) * rnd.choice(pool) * rnd.choice([1, 1, 2])
    return n, ent


def corpus_matrices():
    """[(name, n, {(row, col): value})], deterministic"""
    import random
    rnd = random.Random(CORPUS_SEED)
    blocks = _corpus_blocks(rnd)
    out = []
    # the crafted blocks in both polarities, six or seven blocks to a matrix, in a shuffled order
    both = []
    for lab, col0, m in blocks:
        both.append((lab, col0, m))
        both.append((lab + "_neg", {r: -v for r, v in col0.items()}, m))
    rnd.shuffle(both)
    per = 10
    for t in range(0, len(both), per):
        chunk = both[t:t + per]
        n, ent = _corpus_matrix(rnd, chunk)
        out.append((f"crafted{t // per:02d}", n, ent))
    # a singular column at the end of two crafted matrices
    for t in range(2):
        chunk = both[per * t:per * t + 3]
        n, ent = _corpus_matrix(rnd, chunk, singular=True)
        out.append((f"singular{t}", n, ent))
    for t in range(20):
        n, ent = _corpus_random(rnd)
        out.append((f"random{t:02d}", n, ent))
    return out


def _slab_bytes(arrays):
    import io
    buf = io.BytesIO()
    slabfile.save_to(buf, arrays)
    return buf.getvalue()


def run_corpus():
    import gzip
    import hashlib
    slab, runs, mats = {}, [], []
    with tempfile.TemporaryDirectory() as td:
        for mi, (name, n, ent) in enumerate(corpus_matrices()):
            trip = os.path.join(td, name + ".txt")
            with open(trip, "w") as f:
                f.write(f"{n} {n} {len(ent)}\n")
                for (r, c), v in sorted(ent.items(), key=lambda e: (e[0][1], e[0][0])):
                    f.write(f"{r + 1} {c + 1} {v}\n")
            a_out = os.path.join(td, "a.slab")
            subprocess.check_call([DRIVER, "order", "trip:" + trip, a_out, "0"], stderr=subprocess.DEVNULL)
            a = slabfile.load(a_out)
            assert np.array_equal(a["q"], np.arange(n)), name
            for k in ("Ap", "Ai", "Alen", "Alimbs"):
                slab[f"{name}.{k}"] = a[k]
            mats.append(dict(name=name, n=n, nnz=int(len(a["Ai"]))))
            for pivot in range(6):
                for tol in (CORPUS_TOLS if pivot in (3, 4) else (1.0,)):
                    out = os.path.join(td, "o.slab")
                    subprocess.check_call([DRIVER, "window", "trip:" + trip, out, "0", "0", str(pivot), "0", repr(tol)],
                                          stderr=subprocess.DEVNULL)
                    d = slabfile.load(out)
                    K, status = int(d["K"][0]), int(d["counters"][7])
                    rid = len(runs)
                    slab[f"r{rid:04d}.pinv"] = d["pinv"]
                    runs.append(dict(id=rid, matrix=name, n=n, pivot=pivot, tol=tol, K=K, status=status,
                                     digest=slabfile.factor_digest(d) if K > 0 else None, full=False,
                                     counters={k: int(v) for k, v in zip(
                                         ("N_upd", "B_read", "B_write", "N_src", "L_streamed", "maxlimbs", "K_done"),
                                         d["counters"][:7])}))
    raw = _slab_bytes(slab)
    with open(os.path.join(HERE, "pivot_corpus.slab.gz"), "wb") as f:
        with gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0, compresslevel=9) as g:
            g.write(raw)
    # one record to a line: small, and a diff names the runs that changed
    with open(os.path.join(HERE, "pivot_corpus.json"), "w") as f:
        f.write('{"seed": %d, "tols": %s, "slab_sha256": "%s",\n' % (CORPUS_SEED, json.dumps(list(CORPUS_TOLS)),
                                                                     hashlib.sha256(raw).hexdigest()))
        f.write(' "matrices": [\n  ' + ",\n  ".join(json.dumps(m) for m in mats) + "],\n")
        f.write(' "runs": [\n  ' + ",\n  ".join(json.dumps(r, separators=(",", ":")) for r in runs) + "]}\n")
    print("pivot corpus:", len(mats), "matrices,", len(runs), "runs,",
          sum(r["status"] != 0 for r in runs), "singular")


def main():
    if sys.argv[1:] == ["solve"]:
        run_solve_cases()
        return
    if sys.argv[1:] == ["corpus"]:
        run_corpus()
        return
    names = sys.argv[1:] or list(CASES)
    idx_path = os.path.join(HERE, "index.json")
    index = {}
    if os.path.exists(idx_path):
        index = {e["name"]: e for e in json.load(open(idx_path))}
    for nm in names:
        index[nm] = run_case(nm)
        print(nm, index[nm]["K"], index[nm]["lnz"] + index[nm]["unz"] - index[nm]["K"], index[nm]["digest"])
    json.dump([index[k] for k in CASES if k in index], open(idx_path, "w"), indent=1)


if __name__ == "__main__":
    main()
