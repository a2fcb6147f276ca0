#!/usr/bin/env python3
"""Exact pricing fused on the device (slip_hip_factor_price) against the three-call route on the same operands:
`solve_transpose` (y downloaded), `SparseMatrix.multiply(transpose=True)` (y uploaded again, r = M^T y - det g downloaded) and
`ratio_test` (r uploaded a third time).  Per golden: M is every column of A moved down by one row (ncols = n), and the same
set again with a second shift next to it (ncols = 2n); one problem and eight; nside 1 (Dantzig pricing, sense -1) and 2 (the
dual ratio test).  Right-hand sides and costs are small integers.  One JSON line per configuration: the device ms of the
fused call by pass and of its substitution, the wall time of both routes, the bytes that crossed back on each, the path
counts.  Every number is the median of five calls after a warm-up call of the same kind, except where the warm-up call took
more than one second: then it is that one call.  Complete-run goldens only.
usage: price_probe.py case[,case...]"""
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


def timed(call, read=None):
    """(median wall ms, median of read() after each call, the last result); the warm-up call alone when it took over a second"""
    t0 = time.perf_counter()
    res = call()
    first = (time.perf_counter() - t0) * 1e3
    if first > 1000:
        return first, read() if read else None, res
    walls, reads = [], []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        res = call()
        walls.append((time.perf_counter() - t0) * 1e3)
        if read:
            reads.append(read())
    return statistics.median(walls), [statistics.median(v) for v in zip(*reads)] if read else None, res


def sides_of(rlen, rlimbs, ncols, nprob, nside, dsign):
    """the product's slab as the x slab (and the a slab) of the handle-less ratio test, both times sign(det)"""
    rlen = np.asarray(rlen, np.int32) * np.int32(dsign)
    if nside == 1:
        return (rlen, rlimbs), (None, None)
    off = np.concatenate(([0], np.cumsum(np.abs(rlen.astype(np.int64)))))
    out = []
    for side in (0, 1):
        vecs = [2 * c + side for c in range(nprob)]
        out.append((np.concatenate([rlen[v * ncols:(v + 1) * ncols] for v in vecs]),
                    np.concatenate([rlimbs[off[v * ncols]:off[(v + 1) * ncols]] for v in vecs])))
    return out


for name in sys.argv[1].split(","):
    e, fx = load_case(name)
    n, q = e["n"], np.asarray(fx["q"])
    cols = columns(n, fx["Ap"], fx["Ai"], oracle_lib.bigints(fx["Alen"], fx["Alimbs"]))
    f = sl.Factorization(n, fx["Ap"], fx["Ai"], fx["Alen"], fx["Alimbs"], q, pivot=e["pivot"], tol=e["tol"])
    f.run(0)
    det = oracle_lib.bigints(*f.pivots())[-1]
    dsign = 1 if det > 0 else -1
    for shifts in (1, 2):
        ncols = shifts * n
        mcols = [[((i + 1 + j // n) % n, v) for i, v in cols[j % n].items()] for j in range(ncols)]
        Ap = np.cumsum([0] + [len(c) for c in mcols]).astype(np.int64)
        Ai = np.array([r for c in mcols for r, _ in c], np.int32)
        M = sl.SparseMatrix(n, ncols, Ap, Ai, *slab([v for c in mcols for _, v in c]))
        for nprob in (1, 8):
            for nside in (1, 2):
                nvec = nside * nprob
                rhs = (np.arange(n * nvec, dtype=np.int64) * 2654435761 % (1 << 32)) % 2001 - 1000
                g = (np.arange(ncols * nprob, dtype=np.int64) * 40503 % (1 << 16)) % 201 - 100
                bl, bx = slab(rhs)
                cost = slab(g)
                gfull = np.zeros((nprob, nside, ncols), np.int64)
                gfull[:, 0, :] = g.reshape(nprob, ncols)
                gb, d = slab(gfull.ravel()), slab([det] * nvec)
                sense = -1 if nside == 1 else 1
                back = [0]

                def three():
                    yl, yx = f.solve_transpose(bl, bx, nrhs=nvec)
                    rl, rx = M.multiply(yl, yx, nvec=nvec, transpose=True, b=gb, d=d)
                    x, a = sides_of(rl, rx, ncols, nprob, nside, dsign)
                    back[0] = yl.nbytes + yx.nbytes + rl.nbytes + rx.nbytes + 12 * nprob
                    return sl.ratio_test(ncols, *x, *a, nprob=nprob, sense=sense)

                fused = lambda: f.price(M, bl, bx, nprob=nprob, sides=nside, cost=cost, sense=sense)
                fwall, ms, got = timed(fused, lambda: f.price_ms() + [f.solve_transpose_ms()[0]])
                twall, _, want = timed(three)
                assert all(np.array_equal(u, v) for u, v in zip(got[:3], want)), (name, ncols, nprob, nside)
                print(json.dumps(dict(case=name, n=n, ncols=ncols, nprob=nprob, nside=nside,
                                      gather_width_ms=round(ms[0], 4), scan_ms=round(ms[1], 4), product_ms=round(ms[2], 4),
                                      select_ms=round(ms[3], 4), substitution_ms=round(ms[4], 4),
                                      fused_wall_ms=round(fwall, 3), three_call_wall_ms=round(twall, 3),
                                      fused_bytes_back=16 * nprob, three_call_bytes_back=int(back[0]),
                                      paths=f.price_paths(), best=[int(v) for v in got[0]], vsign=[int(v) for v in got[3]])), flush=True)
        M.close()
    f.close()
