#!/usr/bin/env python3
"""The bounded ratio test fused with its solve (slip_hip_factor_ratio_test_bounded) against today's route on the same handle
-- `solve` with the same two right-hand sides per problem, the whole slab downloaded, the shifted numerators N_i and the
cross-multiplication in Python integers -- and against the unbounded `ratio_test` on the same right-hand sides.  Per golden,
for one problem and for eight, for three sets of bounds:
  unit   kind = 1, lo = 0, den = 1 (ratio_test's own definition: no product is formed),
  box    small integer boxes -5 <= x_i <= 5, den = 1 (one-digit bounds against det),
  own    den = |det| and bounds of the numerators' own size, x_i -+ (3 + i) |alpha_i| of the first problem (the widest
         products the form pass can meet; the steps of the first problem are the distinct integers 3 + i),
the device ms of the form passes (classify, offsets, form) and of the selection, next to that of the substitution of the same
call, the wall ms of the fused call and of today's route, the path counts; and once per problem count the device ms of
ratio_test's selection, its wall ms and the spread (max - min) of both over its five calls.  x side: small integers; a side:
a column of A moved down by one row (both by original row, as `solve` takes them).  Every number is the median of five calls
after a warm-up call of the same kind, except today's route above one second, which is that of the one call.
Complete-run goldens only.
usage: bound_probe.py case[,case...]"""
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


def sample(call, reads):
    """the five samples of every reading (and of the wall ms, last) after one warm-up call"""
    call()
    out = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        call()
        ms = (time.perf_counter() - t0) * 1e3
        out.append([r() for r in reads] + [ms])
    return list(zip(*out))


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


def select(n, num, nprob, det, bnd):
    """the leaving positions from a downloaded slab: the shifted numerators and the cross-multiplication in Python integers,
    sense +1, the smallest index among ties"""
    s, den, best = (1 if det > 0 else -1), bnd["den"], []
    for c in range(nprob):
        xs, avs = num[2 * c * n:(2 * c + 1) * n], num[(2 * c + 1) * n:(2 * c + 2) * n]
        w, Nw, aw = -1, 0, 0
        for i in range(n):
            t = s * avs[i]
            if t > 0 and bnd["kind"][i] & 1:
                N = den * xs[i] - det * bnd["lo"][i]
            elif t < 0 and bnd["kind"][i] & 2:
                N = det * bnd["hi"][i] - den * xs[i]
            else:
                continue
            if w < 0 or s * N * aw < s * Nw * abs(avs[i]):
                w, Nw, aw = i, N, abs(avs[i])
        best.append(w)
    return best


for name in sys.argv[1].split(","):
    e, fx = load_case(name)
    n, q = e["n"], np.asarray(fx["q"])
    cols = columns(n, fx["Ap"], fx["Ai"], oracle_lib.bigints(fx["Alen"], fx["Alimbs"]))
    g = sl.Factorization(n, fx["Ap"], fx["Ai"], fx["Alen"], fx["Alimbs"], q, pivot=e["pivot"], tol=e["tol"])
    g.run(0)
    det = oracle_lib.bigints(*g.pivots())[-1]
    s = 1 if det > 0 else -1
    for nprob in (1, 8):
        flat = []
        for c in range(nprob):
            flat += [int(v) for v in (np.arange(n, dtype=np.int64) * (2654435761 + 2 * c) % (1 << 32)) % 2001 - 1000]
            col = cols[int(q[(n // 3 + 17 * c) % n])]
            flat += [col.get((i + 1) % n, 0) for i in range(n)]
        bl, bx = slab(flat)
        first = oracle_lib.bigints(*g.solve(bl[:2 * n], bx, nrhs=2))
        sets = dict(unit=dict(kind=[1] * n, lo=[0] * n, hi=[0] * n, den=1),
                    box=dict(kind=[3] * n, lo=[-5] * n, hi=[5] * n, den=1),
                    own=dict(kind=[3] * n, lo=[s * first[i] - (3 + i) * abs(first[n + i]) for i in range(n)],
                             hi=[s * first[i] + (3 + i) * abs(first[n + i]) for i in range(n)], den=abs(det)))
        plain = lambda: g.ratio_test(bl, bx, nprob=nprob)
        rs, rw = sample(plain, [g.ratio_test_ms])
        row = dict(case=name, n=n, nprob=nprob, ratio_test_select_ms=round(statistics.median(rs), 4),
                   ratio_test_select_spread_ms=round(max(rs) - min(rs), 4), ratio_test_wall_ms=round(statistics.median(rw), 3),
                   ratio_test_wall_spread_ms=round(max(rw) - min(rw), 3))
        for label, bnd in sets.items():
            bounds = sl.Bounds(n, np.array(bnd["kind"], np.int32), slab(bnd["lo"]), slab(bnd["hi"]), bnd["den"])
            fused = lambda: g.ratio_test_bounded(bl, bx, bounds, nprob=nprob)

            def today():
                xl, xx = g.solve(bl, bx, nrhs=2 * nprob)
                return select(n, oracle_lib.bigints(xl, xx), nprob, det, bnd)

            best, nties, nelig, side = fused()
            assert [int(v) for v in best] == today(), (label, best)
            form, sel, sub, fw = sample(fused, [lambda: g.bound_ms()[0], lambda: g.bound_ms()[1], g.solve_ms])
            row[label] = dict(form_ms=round(statistics.median(form), 4), select_ms=round(statistics.median(sel), 4),
                              substitution_ms=round(statistics.median(sub), 4), fused_wall_ms=round(statistics.median(fw), 3),
                              fused_wall_spread_ms=round(max(fw) - min(fw), 3), today_wall_ms=round(wall(today), 3),
                              paths=g.bound_paths(), neligible=[int(v) for v in nelig], nties=[int(v) for v in nties])
        print(json.dumps(row), flush=True)
    g.close()
