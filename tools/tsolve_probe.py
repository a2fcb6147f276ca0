#!/usr/bin/env python3
"""Kernel time of the transposed solve (slip_hip_factor_solve_transpose) against the plain solve on the same resident factors,
one and sixteen right-hand sides, the build of the transposed view, and the solve time line of both (the phase words of the
debug area: scatter, forward sweep, x * det, back substitution, in microseconds).  Each number is the second call of its kind
(the first one loads the code and, for the transposed solve, builds the view).  Complete-run goldens only.
usage: tsolve_probe.py case[,case...]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import slip_lu_amd as sl  # noqa: E402
from conftest import load_case  # noqa: E402


def phases(g, n):
    w = np.zeros(8, np.int32)
    g.lib.slip_hip_factor_debug_words.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
    if g.lib.slip_hip_factor_debug_words(g.h, 24 * n + 3072, 8, w.ctypes.data) or not w[4]:
        return None
    d = [((int(w[q + 1]) - int(w[q])) & 0xFFFFFFFF) / 100.0 for q in range(4)]
    return dict(scatter_us=round(d[0], 1), forward_us=round(d[1], 1), times_det_us=round(d[2], 1), backward_us=round(d[3], 1))


for name in sys.argv[1].split(","):
    e, fx = load_case(name)
    n, q = e["n"], np.asarray(fx["q"])
    g = sl.Factorization(n, fx["Ap"], fx["Ai"], fx["Alen"], fx["Alimbs"], q, pivot=e["pivot"], tol=e["tol"])
    g.run(0)
    i = g.info()
    b = (np.arange(n, dtype=np.int64) * 2654435761 % (1 << 32)) % 2001 - 1000
    bl, bx = sl.ints_to_slab(b)
    cl, cx = sl.ints_to_slab(b[q])                        # A^T x = b: b by position, b[k] = b_orig[q[k]]
    g.solve(bl, bx)
    g.solve_transpose(cl, cx)
    view_ms = g.solve_transpose_ms()[1]                   # the first transposed solve built the view
    g.solve(bl, bx)
    s1, ph = g.solve_ms(), phases(g, n)
    g.solve_transpose(cl, cx)
    t1, tph = g.solve_transpose_ms()[0], phases(g, n)
    g.solve(np.tile(bl, 16), np.tile(bx, 16), nrhs=16)
    s16 = g.solve_ms()
    g.solve_transpose(np.tile(cl, 16), np.tile(cx, 16), nrhs=16)
    t16 = g.solve_transpose_ms()[0]
    print(json.dumps(dict(case=name, n=n, lnz=i["lnz"], unz=i["unz"], solve_ms=round(s1, 3), tsolve_ms=round(t1, 3),
                          solve16_ms=round(s16, 3), tsolve16_ms=round(t16, 3), view_ms=round(view_ms, 3),
                          phases=ph, tphases=tph)), flush=True)
    g.close()
