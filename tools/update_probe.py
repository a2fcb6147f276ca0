#!/usr/bin/env python3
"""What a change of one column costs with slip_hip_factor_replace_column against what it cost before it (reset + full run),
per case (goldens; a window case keeps its limb cap) and per position p = K/4, K/2, 3K/4, K-1 of the K committed columns
(K = n for a complete run).  One JSON line per (case, position):
  rewind_wall_ms   host wall time of rewind(p) on the complete handle (slip_rewind_kernel's four launches, the state)
  splice_wall_ms   host wall time of replace_column on the handle already rewound: upload of the column, slip_splice_kernel
  update_ms        kernel ms of the run() that follows (columns p..K-1 of the new matrix), and its launches
  full_ms          kernel ms of reset() + run() on the same new matrix: the path there was before
  a_storage        the storage report after the replacement
The new column is the old one with every value v replaced by 3v + 1 (same pattern).  The factors after the update are
compared with those of the full run.
usage: update_probe.py case[,case...]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import oracle_lib  # noqa: E402
import slabfile  # noqa: E402
import slip_lu_amd as sl  # noqa: E402
from conftest import load_case  # noqa: E402


def wall(fn):
    t = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t) * 1e3


for name in [c for c in (sys.argv[1] if len(sys.argv) > 1 else "").split(",") if c]:
    e, fx = load_case(name)
    n, q = e["n"], np.asarray(fx["q"])
    Ap, Ai = np.asarray(fx["Ap"]), np.asarray(fx["Ai"])
    vals = oracle_lib.bigints(fx["Alen"], fx["Alimbs"])
    f = sl.Factorization(n, Ap, Ai, fx["Alen"], fx["Alimbs"], q, pivot=e["pivot"], tol=e["tol"], limb_cap=e["cap"])
    f.run(0, check=False)
    K = f.info()["K"]
    f.reset(); f.run(0, check=False)
    base_ms = f.info()["kernel_ms"]
    print(json.dumps(dict(case=name, n=n, K=K, nnz=int(Ap[n]), full_ms_original=round(base_ms, 3))), flush=True)
    for p in sorted({K // 4, K // 2, (3 * K) // 4, K - 1}):
        j = int(q[p])
        rows = [int(Ai[t]) for t in range(int(Ap[j]), int(Ap[j + 1]))]
        new = [3 * vals[t] + 1 for t in range(int(Ap[j]), int(Ap[j + 1]))]
        _, t_rewind = wall(lambda: f.rewind(min(p, f.info()["K"])))       # (a window that ended before p: nothing to undo)
        _, t_splice = wall(lambda: f.replace_column(j, rows, new))
        rc = f.run(0, check=False)
        i = f.info()
        upd = slabfile.factor_digest(f.download()) if i["K"] > 0 else None
        f.reset(); rc2 = f.run(0, check=False)
        i2 = f.info()
        same = (slabfile.factor_digest(f.download()) if i2["K"] > 0 else None) == upd and (rc, i["K"]) == (rc2, i2["K"])
        print(json.dumps(dict(case=name, position=p, column=j, nz=len(rows), rewind_wall_ms=round(t_rewind, 3),
                              splice_wall_ms=round(t_splice, 3), update_ms=round(i["kernel_ms"], 3), launches=i["launches"],
                              full_ms=round(i2["kernel_ms"], 3), status=rc, K_after=i["K"], identical=bool(same),
                              a_storage=f.a_storage())), flush=True)
    f.close()
