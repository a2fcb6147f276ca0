#!/usr/bin/env python3
"""The exact ratio test fused with its solve (slip_hip_factor_ratio_test) against today's route on the same handle: `solve`
with the same two right-hand sides per problem, the whole slab downloaded, the selection in Python integers on it.  Per
golden, for one problem and for eight: the device time of the selection kernels (bound pass, filter, folds) next to that of
the substitution that precedes them in the same call, the wall time of both routes, the bytes that cross back, and the four
path counts.  x side: small integers; a side: a column of A moved down by one row, so that it is no column of the basis
(both by original row, as `solve` takes them).  Every number is
the median of five calls after a warm-up call of the same kind, except a wall time above one second (today's route on the
large cases), which is that of the one call.  Complete-run goldens only.
usage: ratio_probe.py case[,case...]"""
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
from check_helpers import columns, slab  # noqa: E402
from conftest import load_case  # noqa: E402

REPEATS = 5


def median(call, read):
    call()
    out = []
    for _ in range(REPEATS):
        call()
        out.append(read())
    return statistics.median(out) if not isinstance(out[0], list) else [statistics.median(v) for v in zip(*out)]


def wall(call):
    t0 = time.perf_counter()
    call()
    first = (time.perf_counter() - t0) * 1e3
    if first > 1000:
        return first
    out = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        call()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def select(n, num, nprob, dsign):
    """the leaving positions from a downloaded slab: cross-multiplication in Python integers, sense +1, the smallest index
    among ties"""
    best = []
    for c in range(nprob):
        xs, avs = num[2 * c * n:(2 * c + 1) * n], num[(2 * c + 1) * n:(2 * c + 2) * n]
        w = -1
        for i in range(n):
            if dsign * avs[i] <= 0:
                continue
            if w < 0 or dsign * xs[i] * abs(avs[w]) < dsign * xs[w] * abs(avs[i]):
                w = i
        best.append(w)
    return best


for name in sys.argv[1].split(","):
    e, fx = load_case(name)
    n, q = e["n"], np.asarray(fx["q"])
    cols = columns(n, fx["Ap"], fx["Ai"], oracle_lib.bigints(fx["Alen"], fx["Alimbs"]))
    g = sl.Factorization(n, fx["Ap"], fx["Ai"], fx["Alen"], fx["Alimbs"], q, pivot=e["pivot"], tol=e["tol"])
    g.run(0)
    dsign = 1 if oracle_lib.bigints(*g.pivots())[-1] > 0 else -1
    row = dict(case=name, n=n)
    for nprob in (1, 8):
        flat = []
        for c in range(nprob):
            flat += [int(v) for v in (np.arange(n, dtype=np.int64) * (2654435761 + 2 * c) % (1 << 32)) % 2001 - 1000]
            col = cols[int(q[(n // 3 + 17 * c) % n])]
            flat += [col.get((i + 1) % n, 0) for i in range(n)]
        bl, bx = slab(flat)

        def today():
            xl, xx = g.solve(bl, bx, nrhs=2 * nprob)
            return select(n, oracle_lib.bigints(xl, xx), nprob, dsign), xl.nbytes + xx.nbytes

        fused = lambda: g.ratio_test(bl, bx, nprob=nprob)
        best, nties, nelig = fused()
        want, slab_bytes = today()
        assert [int(v) for v in best] == want, (best, want)
        s = "" if nprob == 1 else "8"
        row.update({"select%s_ms" % s: round(median(fused, g.ratio_test_ms), 4),
                    "substitution%s_ms" % s: round(median(fused, g.solve_ms), 4),
                    "fused_wall%s_ms" % s: round(wall(fused), 3), "today_wall%s_ms" % s: round(wall(today), 3),
                    "solve_only_wall%s_ms" % s: round(wall(lambda: g.solve(bl, bx, nrhs=2 * nprob)), 3),
                    "bytes_back%s" % s: 12 * nprob, "solve_slab_bytes%s" % s: int(slab_bytes),
                    "paths%s" % s: g.ratio_test_paths(), "nties%s" % s: [int(v) for v in nties], "neligible%s" % s: [int(v) for v in nelig]})
    print(json.dumps(row), flush=True)
    g.close()
