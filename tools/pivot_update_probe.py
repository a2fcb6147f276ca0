#!/usr/bin/env python3
"""The exact step fused with its solve (slip_hip_factor_step) against the route without it on the same handle -- `ratio_test`
on the same two right-hand sides per problem, then a second `solve` of the x sides, the substitution a caller repeats on the
new factors to learn the new basic solution (timed here on the handle as it stands: the same matrix size and fill).  Per golden,
for one problem and for sixteen: the device ms of the update's passes (classify, offsets, form) and of its selection, next to
the device ms of the substitution of the same call and of the second substitution it replaces; the wall ms of the step and of
the route without it; the path counts.  x side: small integers; a side: A(:,q) w for a small integer w (its solve is det * w, so
every problem has eligible entries).  Every number is the median of five calls after a warm-up call of the same kind, with the
spread (max - min) of the five.  Complete-run goldens only.
usage: pivot_update_probe.py case[,case...]"""
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


def med(v, nd=4):
    return [round(statistics.median(v), nd), round(max(v) - min(v), nd)]


for name in sys.argv[1].split(","):
    e, fx = load_case(name)
    n, q = e["n"], np.asarray(fx["q"])
    cols = columns(n, fx["Ap"], fx["Ai"], oracle_lib.bigints(fx["Alen"], fx["Alimbs"]))
    g = sl.Factorization(n, fx["Ap"], fx["Ai"], fx["Alen"], fx["Alimbs"], q, pivot=e["pivot"], tol=e["tol"])
    g.run(0)
    det = oracle_lib.bigints(*g.pivots())[-1]
    for nprob in (1, 16):
        flat, xs = [], []
        for c in range(nprob):
            x = [int(v) for v in (np.arange(n, dtype=np.int64) * (2654435761 + 2 * c) % (1 << 32)) % 2001 - 1000]
            a = [0] * n
            for k in range(n):
                w = (7 * k + c) % 5 - 1
                if w:
                    for i, v in cols[int(q[k])].items():
                        a[i] += v * w
            flat += x + a; xs += x
        bl, bx = slab(flat)
        xl, xx = slab(xs)
        step = lambda: g.step(bl, bx, nprob=nprob)

        def without():
            g.ratio_test(bl, bx, nprob=nprob)
            g.solve(xl, xx, nrhs=nprob)

        res = step()
        assert all(int(v) >= 0 for v in res.best) and not any(res.ninexact)
        form, sel, sub, sw = sample(step, [lambda: g.update_ms()[0], lambda: g.update_ms()[1], g.solve_ms])
        rsel, again, ww = sample(without, [g.ratio_test_ms, g.solve_ms])
        first = sample(lambda: g.ratio_test(bl, bx, nprob=nprob), [g.solve_ms])[0]
        print(json.dumps(dict(case=name, n=n, det_digits=(abs(det).bit_length() + 31) // 32, nprob=nprob,
                              update_form_ms=med(form), update_select_ms=med(sel), step_substitution_ms=med(sub, 3),
                              ratio_test_select_ms=med(rsel), ratio_test_substitution_ms=med(first, 3),
                              second_substitution_ms=med(again, 3), step_wall_ms=med(sw, 3), without_wall_ms=med(ww, 3),
                              paths=g.update_paths(), result_limbs=int(res.x[1].size))), flush=True)
    g.close()
