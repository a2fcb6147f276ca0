#!/usr/bin/env python3
"""Device time of the exact product r = A(:,q) x - det b (slip_hip_factor_multiply) against the check on identical operands
(slip_hip_factor_check: the same multiply-accumulate work without the width pass, the store and the pack) and against the
same residual in Python integers on the host, one and sixteen vectors, x the solve's own numerators.  The product's time is
split by pass (widths, offset scans, products, packing).  Every device number is the median of five calls after a warm-up
call of the same kind.  Complete-run goldens only.
usage: product_probe.py case[,case...]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import oracle_lib  # noqa: E402
import slip_lu_amd as sl  # noqa: E402
from check_helpers import columns, residual  # noqa: E402
from conftest import load_case  # noqa: E402

REPEATS = 5


def median(call, read):
    call()
    out = []
    for _ in range(REPEATS):
        call()
        out.append(read())
    return statistics.median(out) if not isinstance(out[0], list) else [statistics.median(v) for v in zip(*out)]


for name in sys.argv[1].split(","):
    e, fx = load_case(name)
    n, q = e["n"], np.asarray(fx["q"])
    g = sl.Factorization(n, fx["Ap"], fx["Ai"], fx["Alen"], fx["Alimbs"], q, pivot=e["pivot"], tol=e["tol"])
    g.run(0)
    b = (np.arange(n, dtype=np.int64) * 2654435761 % (1 << 32)) % 2001 - 1000
    row = dict(case=name, n=n, nnz=int(fx["Ap"][n]))
    for nvec in (1, 16):
        bl, bx = sl.ints_to_slab(np.tile(b, nvec))
        xl, xx = g.solve(bl, bx, nrhs=nvec)
        row["x_limbs_max"] = int(np.abs(xl).max())
        check = median(lambda: g.check(bl, bx, xl, xx, nrhs=nvec), g.check_ms)
        total = median(lambda: g.multiply(xl, xx, nvec=nvec, b=(bl, bx)), g.multiply_ms)
        passes = median(lambda: g.multiply(xl, xx, nvec=nvec, b=(bl, bx)), sl.multiply_passes)
        alone = median(lambda: g.multiply(xl, xx, nvec=nvec), lambda: sl.multiply_passes()[2])
        rlen, _ = g.multiply(xl, xx, nvec=nvec, b=(bl, bx))
        assert not rlen.any()
        s = "" if nvec == 1 else "16"
        row.update({"check%s_ms" % s: round(check, 3), "multiply%s_ms" % s: round(total, 3),
                    "passes%s_ms" % s: [round(v, 3) for v in passes], "product_pass_no_b%s_ms" % s: round(alone, 3)})
    # the same residual of one vector on the host: Python integers, operands already converted
    vals = oracle_lib.bigints(fx["Alen"], fx["Alimbs"])
    cols = columns(n, fx["Ap"], fx["Ai"], vals)
    x = oracle_lib.bigints(*g.solve(*sl.ints_to_slab(b)))
    det = oracle_lib.bigints(*g.pivots())[-1]
    xcol = [0] * n
    for p in range(n):
        xcol[int(q[p])] = x[p]
    t0 = time.perf_counter()
    r = residual(n, cols, xcol, det, [int(v) for v in b])
    row["host_python_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    assert not any(r)
    print(json.dumps(row), flush=True)
    g.close()
