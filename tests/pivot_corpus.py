"""The pivot-edge corpus (tests/golden/pivot_corpus.json, pivot_corpus.slab.gz): small signed matrices built so that
slip_get_pivot's decisions fall on signs, ties and exact tolerance ratios, with the compiled reference's result for
every pivoting scheme (schemes 3 and 4 under several tolerances).  Made by `make_golden.py corpus`."""
import json
import os

import numpy as np

import slabfile
from conftest import GOLDEN, check_against_golden

_CACHE = {}


def corpus():
    """(index dict, slab dict), loaded once"""
    if "c" not in _CACHE:
        idx = json.load(open(os.path.join(GOLDEN, "pivot_corpus.json")))
        _CACHE["c"] = (idx, slabfile.load(os.path.join(GOLDEN, "pivot_corpus.slab.gz")))
    return _CACHE["c"]


def matrix(name):
    """(n, Ap, Ai, Alen, Alimbs, q) of one corpus matrix, as the reference holds it; column order 0"""
    idx, slab = corpus()
    n = {m["name"]: m for m in idx["matrices"]}[name]["n"]
    return (n, slab[name + ".Ap"], slab[name + ".Ai"], slab[name + ".Alen"], slab[name + ".Alimbs"],
            np.arange(n, dtype=np.int32))


def runs(pivots=None, matrices=None):
    idx, _ = corpus()
    return [r for r in idx["runs"] if (pivots is None or r["pivot"] in pivots) and (matrices is None or r["matrix"] in matrices)]


def check_run(run, res):
    """res (an implementation's canonical factor dict) against the reference's record of `run`: the status, the columns
    done, pinv, the SHA-256 over L, U, rho, pinv; the algorithmic counters of complete runs"""
    _, slab = corpus()
    assert res["status"] == run["status"], (res["status"], run["status"])
    check_against_golden(run, {"pinv": slab["r%04d.pinv" % run["id"]]}, res, counters=run["status"] == 0)


def label(run):
    return "%s-p%d-tol%g" % (run["matrix"], run["pivot"], run["tol"])
