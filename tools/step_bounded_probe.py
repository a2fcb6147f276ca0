#!/usr/bin/env python3
"""The bounded step fused with its solve (slip_hip_factor_step_bounded) against the two routes without it on the same handle
and the same operands:
  A  `ratio_test_bounded` with the winners' slab, a `solve` of the same right-hand sides that downloads both numerator
     vectors, P and T formed on the host, `pivot_update` on the downloaded slabs;
  B  `ratio_test_bounded`, then a second `solve` of nprob right-hand sides (timed on the handle as it stands: the same matrix
     size and fill as the substitution a caller runs for the next iterate).
Per golden, for one problem and for sixteen, and for a call whose problems all pivot (a finite range that does not block) and
one whose problems all flip (range 0): the device ms of the four passes (the selection's form passes, the selection,
slip_bstep_kernel, the update) and of the substitution of the same call; the wall ms of the step and of both routes; the path
counts.  x side: small integers; a side: A(:,q) w for a small integer w; bounds: the box floor(x_i) - 3 .. floor(x_i) + 4
around the true values, den 1.  Every number is the median of five calls after a warm-up call of the same kind, with the
spread (max - min) of the five.  Complete-run goldens only.
The kinds run in the order given (default pivot,flip).
usage: step_bounded_probe.py case[,case...] [kind[,kind]]"""
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
KINDS = dict(pivot=10 ** 12, flip=0)                         # the range er of every problem


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
            x = [int(v) for v in (np.arange(n, dtype=np.int64) * 2654435761 % (1 << 32)) % 2001 - 1000]      # (one x: the box holds for all)
            a = [0] * n
            for k in range(n):
                w = (7 * k + c) % 5 - 1
                if w:
                    for i, v in cols[int(q[k])].items():
                        a[i] += v * w
            flat += x + a; xs += x
        bl, bx = slab(flat)
        xl, xx = slab(xs)
        base = [v // det for v in oracle_lib.bigints(*g.solve(xl, xx, nrhs=nprob))[:n]]
        bnd = sl.Bounds(n, np.full(n, 3, np.int32), slab([v - 3 for v in base]), slab([v + 4 for v in base]))
        for kind in (sys.argv[2] if len(sys.argv) > 2 else "pivot,flip").split(","):
            er = KINDS[kind]
            ent = sl.Entering(nprob, [1] * nprob, er, 2)
            step = lambda: g.step_bounded(bl, bx, bnd, ent, nprob=nprob)

            def route_a():
                sel = g.ratio_test_bounded(bl, bx, bnd, nprob=nprob, winners=True)
                num = oracle_lib.bigints(*g.solve(bl, bx, nrhs=2 * nprob))
                win = oracle_lib.bigints(sel[4], sel[5])
                v = [t for c in range(nprob) for t in num[2 * c * n:(2 * c + 1) * n]]
                a = [t for c in range(nprob) for t in num[(2 * c + 1) * n:(2 * c + 2) * n]]
                if kind == "pivot":
                    P, T, D = [win[2 * c + 1] for c in range(nprob)], [win[2 * c] for c in range(nprob)], [det] * nprob
                else:
                    P, T, D = [1] * nprob, [er] * nprob, None
                return sl.pivot_update(n, *slab(v), *slab(a), slab(P), slab(T), d=None if D is None else slab(D), nprob=nprob)

            def route_b():
                g.ratio_test_bounded(bl, bx, bnd, nprob=nprob)
                g.solve(xl, xx, nrhs=nprob)

            res = step()
            assert all(int(m) == (1 if kind == "pivot" else 2) for m in res.move) and not any(res.ninexact), (kind, res.move)
            ms = lambda k: (lambda: g.step_bounded_ms()[k])
            form, sel, scal, upd, sub, sw = sample(step, [ms(0), ms(1), ms(2), ms(3), g.solve_ms])
            aw = sample(route_a, [])[0]
            second, bw = sample(route_b, [g.solve_ms])
            print(json.dumps(dict(case=name, n=n, det_digits=(abs(det).bit_length() + 31) // 32, nprob=nprob, moves=kind,
                                  select_form_ms=med(form), select_ms=med(sel), scalars_ms=med(scal), update_ms=med(upd),
                                  substitution_ms=med(sub, 3), second_substitution_ms=med(second, 3),
                                  step_wall_ms=med(sw, 3), route_a_wall_ms=med(aw, 3), route_b_wall_ms=med(bw, 3),
                                  paths=g.step_bounded_paths(), result_limbs=int(res.x[1].size))), flush=True)
    g.close()
