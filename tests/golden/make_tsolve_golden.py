#!/usr/bin/env python3
"""Generate the transposed-solve fixtures tests/golden/tsolve_*.slab.gz + tsolve_index.json from the COMPILED REFERENCE.

The reference has no transposed solve, but the rational solution of A^T x = b is unique: this script writes A^T of a solve
golden's matrix (the matrix slip_hip_factor_create factorises: a row repeated in a column keeps its LAST value) as a 1-based
triplet file and runs oracle/_ref/ref_driver in its `solve` mode on it -- the reference's own SLIP_LU_analyze +
SLIP_LU_factorize + SLIP_LU_solve for the deterministic right-hand side b_i = ((i*2654435761) mod 2001) - 1000.  Each
fixture keeps the driver's column order q_T of A^T and the solution before SLIP_permute_x:
x[q_T[p]] = xnum[p] / xden[p] solves A^T x = b.  The matrix itself is not stored again: `source` names the solve golden
(tests/golden/solve_index.json) it comes from.

Runs only where the reference was built (oracle/Makefile `ref`).  Usage:  python tests/golden/make_tsolve_golden.py
"""
import gzip
import io
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib  # noqa: E402
import slabfile  # noqa: E402
from conftest import solve_inputs  # noqa: E402

DRIVER = os.path.join(ROOT, "oracle", "_ref", "ref_driver")
CASES = {"tsolve_test_mat": "solve_test_mat", "tsolve_10teams": "solve_10teams", "tsolve_gen_n40": "solve_gen_n40"}


def transpose_triplet(path, n, Ap, Ai, vals):
    """A^T as 1-based triplet text: entry (i, j) of A goes to (j, i), the last of a repeated row of a column only"""
    ent = {}
    for j in range(n):
        for p in range(int(Ap[j]), int(Ap[j + 1])):
            ent[(j, int(Ai[p]))] = vals[p]                      # (row of A^T, column of A^T)
    with open(path, "w") as f:
        f.write(f"{n} {n} {len(ent)}\n")
        for (r, c), v in sorted(ent.items(), key=lambda e: (e[0][1], e[0][0])):
            f.write(f"{r + 1} {c + 1} {v}\n")


def main():
    solve_cases = {c["name"]: c for c in json.load(open(os.path.join(HERE, "solve_index.json")))}
    idx = []
    with tempfile.TemporaryDirectory() as td:
        for name, src in CASES.items():
            n, Ap, Ai, Alen, Alimbs, _, _ = solve_inputs(solve_cases[src])
            trip, out = os.path.join(td, name + ".txt"), os.path.join(td, "s.slab")
            transpose_triplet(trip, n, Ap, Ai, oracle_lib.bigints(Alen, Alimbs))
            subprocess.check_call([DRIVER, "solve", "trip:" + trip, out], stderr=subprocess.DEVNULL)
            d = slabfile.load(out)
            assert int(d["n"][0]) == n and int(d["K"][0]) == n, name
            buf = io.BytesIO()
            slabfile.save_to(buf, {k: d[k] for k in ("q", "xnumlen", "xnumlimbs", "xdenlen", "xdenlimbs")})
            with open(os.path.join(HERE, name + ".slab.gz"), "wb") as f:
                with gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0, compresslevel=9) as g:
                    g.write(buf.getvalue())
            idx.append(dict(name=name, source=src, n=n))
            print(name, n, os.path.getsize(os.path.join(HERE, name + ".slab.gz")), "bytes")
    json.dump(idx, open(os.path.join(HERE, "tsolve_index.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
