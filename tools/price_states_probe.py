#!/usr/bin/env python3
"""Pricing with nonbasic states and reference weights (slip_hip_factor_price_states) next to slip_hip_factor_price on the same
handle, matrix and right-hand sides, in one session.  Per golden: M is every column of A moved down by one row (ncols = n), as
tools/price_probe.py builds it; one problem and eight; nside 1, sense -1, small integer right-hand sides and costs; the states
cycle through 1, 2, 3, 0.  Three rules: Dantzig with states (no weights), weights of one digit, weights of det's size.  One
JSON line per configuration and rule: the device ms of the classify, offset and square passes and of the selection, of the
substitution of the same call, the path counts, the wall time; and one line for `price` itself with the device ms of its four
passes and of its substitution.  Every figure is the median of five calls after a warm-up call of the same kind, with max -
min of the five next to it.  (The products of a price_states call are slip_product_kernel launches on the same operands as
price's and are not timed apart: price's product_ms is their figure.)  Complete-run goldens only.
usage: price_states_probe.py case[,case...]"""
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


def timed(call, read):
    """per figure of read() (the wall ms first): (median, max - min) over five calls after a warm-up call; the last result"""
    res = call()
    rows = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        res = call()
        rows.append([(time.perf_counter() - t0) * 1e3] + read())
    return [(round(statistics.median(v), 4), round(max(v) - min(v), 4)) for v in zip(*rows)], res


for name in sys.argv[1].split(","):
    e, fx = load_case(name)
    n, q = e["n"], np.asarray(fx["q"])
    cols = columns(n, fx["Ap"], fx["Ai"], oracle_lib.bigints(fx["Alen"], fx["Alimbs"]))
    f = sl.Factorization(n, fx["Ap"], fx["Ai"], fx["Alen"], fx["Alimbs"], q, pivot=e["pivot"], tol=e["tol"])
    f.run(0)
    det = abs(oracle_lib.bigints(*f.pivots())[-1])
    ncols = n
    mcols = [[((i + 1) % n, v) for i, v in cols[j].items()] for j in range(ncols)]
    Ap = np.cumsum([0] + [len(c) for c in mcols]).astype(np.int64)
    Ai = np.array([r for c in mcols for r, _ in c], np.int32)
    M = sl.SparseMatrix(n, ncols, Ap, Ai, *slab([v for c in mcols for _, v in c]))
    state = np.array([(j + 1) % 4 for j in range(ncols)], np.int32)
    rules = (("dantzig", None), ("w_one_digit", slab([1 + (j * 2654435761) % 65521 for j in range(ncols)])),
             ("w_det_size", slab([det + j for j in range(ncols)])))
    for nprob in (1, 8):
        rhs = (np.arange(n * nprob, dtype=np.int64) * 2654435761 % (1 << 32)) % 2001 - 1000
        g = (np.arange(ncols * nprob, dtype=np.int64) * 40503 % (1 << 16)) % 201 - 100
        bl, bx = slab(rhs)
        cost = slab(g)
        fig, got = timed(lambda: f.price(M, bl, bx, nprob=nprob, sides=1, cost=cost, sense=-1),
                         lambda: f.price_ms() + [f.solve_transpose_ms()[0]])
        keys = ("wall_ms", "gather_width_ms", "scan_ms", "product_ms", "select_ms", "substitution_ms")
        print(json.dumps(dict(case=name, n=n, ncols=ncols, nprob=nprob, rule="price", det_digits=(det.bit_length() + 31) // 32,
                              **{k: v[0] for k, v in zip(keys, fig)}, **{k + "_spread": v[1] for k, v in zip(keys, fig)},
                              paths=f.price_paths(), best=[int(v) for v in got[0]])), flush=True)
        for rule, wt in rules:
            fig, got = timed(lambda: f.price_states(M, bl, bx, state, weights=wt, nprob=nprob, sides=1, cost=cost, sense=-1),
                             lambda: f.price_states_ms() + [f.solve_transpose_ms()[0]])
            keys = ("wall_ms", "classify_square_ms", "select_ms", "substitution_ms")
            print(json.dumps(dict(case=name, n=n, ncols=ncols, nprob=nprob, rule=rule,
                                  **{k: v[0] for k, v in zip(keys, fig)}, **{k + "_spread": v[1] for k, v in zip(keys, fig)},
                                  paths=f.price_states_paths(), best=[int(v) for v in got[0]], neligible=[int(v) for v in got[2]])), flush=True)
    M.close()
    f.close()
