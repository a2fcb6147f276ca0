#!/usr/bin/env python3
"""Solve straight to doubles (slip_hip_factor_solve_double) against the numerators-then-divide route it replaces, on resident
factors, one and sixteen right-hand sides.  Per case and nrhs, one JSON line:
  solve_ms / to_double_ms   device ms of the substitution and of the conversion kernel of the same solve_double call
  wave_share                share of the entries the lane pass left to the exact wave pass
  on_grid_share             share of the entries whose exact value IS a nonzero double (integers, dyadic fractions): these always
                            take the wave pass, leading bits cannot tell them from their lower neighbour
  double_wall_ms            host wall time of solve_double
  solve_wall_ms             host wall time of solve (numerators to the host) for the same right-hand sides
  divide_wall_ms            one exact truncated division per entry on the host (tests/todouble_helpers.py:trunc_double, Python
                            integers) -- what a caller of solve still has to do
  d2h_double / d2h_solve    bytes handed back to the caller: 8 per entry, against 4 per entry + the numerators' limbs
Each timed call is the second of its kind (the first loads the code and sizes the buffers).  The doubles of both routes are
compared bit for bit.  Complete-run goldens only.
usage: todouble_probe.py case[,case...]"""
import json
import os
import sys
import time
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import oracle_lib  # noqa: E402
import slip_lu_amd as sl  # noqa: E402
from conftest import load_case  # noqa: E402
from todouble_helpers import bits, trunc_double  # noqa: E402


def wall(fn):
    t = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t) * 1e3


for name in sys.argv[1].split(","):
    e, fx = load_case(name)
    n, q = e["n"], np.asarray(fx["q"])
    g = sl.Factorization(n, fx["Ap"], fx["Ai"], fx["Alen"], fx["Alimbs"], q, pivot=e["pivot"], tol=e["tol"])
    g.run(0)
    det = oracle_lib.bigints(*g.pivots())[-1]
    b = (np.arange(n, dtype=np.int64) * 2654435761 % (1 << 32)) % 2001 - 1000
    bl, bx = sl.ints_to_slab(b)
    for nrhs in (1, 16):
        cl, cx = np.tile(bl, nrhs), np.tile(bx, nrhs)
        g.solve_double(cl, cx, nrhs=nrhs)
        got, dwall = wall(lambda: g.solve_double(cl, cx, nrhs=nrhs))
        solve_ms, conv_ms, slow = g.solve_ms(), g.to_double_ms(), g.to_double_slow()
        g.solve(cl, cx, nrhs=nrhs)
        (xlen, xlimbs), swall = wall(lambda: g.solve(cl, cx, nrhs=nrhs))
        x = oracle_lib.bigints(xlen[:n], xlimbs)                      # the first right-hand side: the others repeat it
        want, divwall = wall(lambda: [trunc_double(v, det) for v in x])
        on_grid = sum(1 for v, w in zip(x, want) if v and Fraction(w) * det == v)
        same = all(bits(got[0, int(q[p])]) == bits(want[p]) for p in range(n))
        print(json.dumps(dict(case=name, n=n, nrhs=nrhs, det_limbs=(det.bit_length() + 63) // 64, solve_ms=round(solve_ms, 3),
                              to_double_ms=round(conv_ms, 3), wave_share=round(slow / (n * nrhs), 4), on_grid_share=round(on_grid / n, 4),
                              double_wall_ms=round(dwall, 2), solve_wall_ms=round(swall, 2), divide_wall_ms=round(divwall * nrhs, 2),
                              d2h_double=8 * n * nrhs, d2h_solve=int(4 * n * nrhs + 8 * xlimbs.size), identical=same)), flush=True)
    g.close()
