#!/usr/bin/env python3
"""Development probe of the factorisation on golden cases (tests/golden): timing, parity, path counters.

  probe.py run CASE[,CASE...] [--workers W,...] [--waves V,...] [--flags F,...] [--lib PATH]
      every case x flags x waves x workers: one handle, a first run (creation and wall time, launches, digest parity)
      and a second run on the same handle (kernel time, us per column, bytes, GB/s, the path counters); one JSON line each
  probe.py repeat CASE [--reps R] [--shapes WAVES:WORKERS:FLAGS,...] [--fresh] [--lib PATH]
      R runs per launch shape on one handle (--fresh: a new handle per run), one line per run; a run whose factors
      differ from the golden digest is compared array by array with the CPU oracle (first differing entries, columns)
  probe.py commits CASE[,CASE...] [--workers W] [--waves V] [--flags F,...]
      the columns the short chain / the committer / the chain engine took, and the kernel time, per flag set
      (default 0,4,2: everything; no helping with update queues; no committer workgroup)

--flags are the diagnostic bits of slip_hip_options.reserved (include/slip_hip.h); --lib loads another build of the
library (csrc/Makefile: `make prof`, `make cprof`).

The scripts this one replaces:
  gpu_probe.py CASE@WAVES ...           -> run CASES --waves V          (digest parity, timings, GB/s, speedup vs the reference)
  worker_probe.py CASES W,.. [V,..]     -> run CASES --workers W,.. --waves V,..
  waves_probe.py CASES V,..             -> run CASES --waves V,..
  helper_probe.py CASES H,..            -> dropped: its helper count and fork_min were launch options that no longer exist
  flags_probe.py CASES F,.. [reps] [W]  -> run CASES --flags F,.. --workers W, or repeat CASE --shapes 0:W:F --reps R
  w2_probe.py CASE V W R [F]            -> repeat CASE --shapes V:W:F --reps R --fresh  (handle reuse: without --fresh)
  commit_probe.py CASES [W] [V]         -> commits CASES --workers W --waves V
  diff_probe.py CASES [W] [V]           -> repeat CASE --shapes V:W:0 --reps 1  (oracle comparison of a differing run)
  race_probe.py CASE R [LIB] [SHAPES]   -> repeat CASE --reps R --lib LIB --shapes ...
  race_diff.py CASE R W                 -> repeat CASE --reps R --shapes 0:W:0
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import slabfile  # noqa: E402
from conftest import load_case  # noqa: E402
import slip_lu_amd as sl  # noqa: E402

ARRAYS = ("pinv", "Lp", "Up", "Li", "Ui", "Llen", "Ulen", "rholen", "Llimbs", "Ulimbs", "rholimbs")


def ints(s):
    return [int(x) for x in str(s).split(",")]


def handle(entry, fix, waves=0, workers=0, flags=0, lib=None):
    return sl.Factorization(entry["n"], fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"], pivot=entry["pivot"],
                            tol=entry["tol"], limb_cap=entry["cap"], waves=waves, workers=workers, debug_flags=flags, lib_path=lib)


def counters(i):
    return dict(short=i["short_commits"], committer=i["committer_commits"], engine=i["engine_commits"],
                engine_sources=i["engine_sources"], retract=i["retractions"], reexport=i["reexports"],
                farm_jobs=i["farm_jobs"], farm_items=i["farm_items"])


def parity(f, entry):
    return slabfile.factor_digest(f.download()) == entry["digest"] if f.info()["K"] > 0 else None


def cmd_run(a):
    for name in a.cases.split(","):
        entry, fix = load_case(name)
        for flags in ints(a.flags):
            for waves in ints(a.waves):
                for workers in ints(a.workers):
                    t0 = time.time()
                    f = handle(entry, fix, waves, workers, flags, a.lib)
                    t1 = time.time()
                    rc1 = f.run(entry["kmax"], check=False)
                    t2 = time.time()
                    i1 = f.info()
                    ok = parity(f, entry)
                    f.reset()
                    rc = f.run(entry["kmax"], check=False)
                    i = f.info()
                    f.close()
                    ms = max(i["kernel_ms"], 1e-9)
                    nnz = i["lnz"] + i["unz"] - i["K"]
                    print(json.dumps(dict(
                        case=name, flags=flags, waves=i["waves"], workers=i["workers"], rc=rc1, rc_2nd=rc, K=i["K"], parity=ok,
                        ok=i["K"] == entry["K"] and i["b_read"] == entry["counters"]["B_read"],
                        create_ms=round((t1 - t0) * 1e3, 1), run_wall_ms=round((t2 - t1) * 1e3, 1),
                        kernel_ms_1st=round(i1["kernel_ms"], 3), launches_1st=i1["launches"], xcap_1st=i1["xcap_digits"],
                        kernel_ms=round(i["kernel_ms"], 3), launches=i["launches"], us_per_col=round(1e3 * ms / max(i["K"], 1), 2),
                        knnz_per_s=round(nnz / ms, 1), b_read=i["b_read"], b_write=i["b_write"], gbs=round(i["b_read"] / ms / 1e6, 3),
                        ref_ms=round(entry["ref_seconds"] * 1e3, 2), speedup_vs_ref=round(entry["ref_seconds"] * 1e3 / ms, 2),
                        **counters(i))), flush=True)


def oracle_diff(entry, fix, got):
    """where the factors differ from the CPU oracle: per array, the first differing entries (and their columns)"""
    import oracle_lib
    ref = oracle_lib.factorize(entry["n"], fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"], pivot=entry["pivot"],
                               kmax=entry["kmax"], cap=entry["cap"], tol=entry["tol"])
    print("  K", got["K"], "oracle", ref["K"])
    for k in ARRAYS:
        x, y = np.asarray(got[k]).astype(np.int64), np.asarray(ref[k]).astype(np.int64)
        if x.shape != y.shape:
            print("  ", k, "shape", x.shape, y.shape)
            continue
        d = np.nonzero(x != y)[0]
        if not len(d):
            continue
        print("  ", k, "differs at", len(d), "of", len(x), "first", d[:8], "got", x[d[:4]], "want", y[d[:4]])
        if k in ("Li", "Llen", "Ui", "Ulen"):
            P = np.asarray(ref["Lp" if k[0] == "L" else "Up"])
            cols = np.unique(np.searchsorted(P, d, side="right") - 1)
            print("      columns", cols[:10], "count", len(cols), "col sizes", [int(P[c + 1] - P[c]) for c in cols[:5]])
        if k == "pinv":
            print("      rows", d[:6], "oracle pos", y[d[:6]], "got pos", x[d[:6]])
    print("   counters got", list(got["counters"]), "oracle", list(ref["counters"]))


def cmd_repeat(a):
    entry, fix = load_case(a.case)
    for shape in a.shapes.split(","):
        waves, workers, flags = (int(x) for x in shape.split(":"))
        f, nbad = None, 0
        for rep in range(a.reps):
            if f is None:
                f = handle(entry, fix, waves, workers, flags, a.lib)
            else:
                f.reset()
            rc = f.run(entry["kmax"], check=False)
            i = f.info()
            d = f.download()
            ok = rc == 0 and d["K"] == entry["K"] and slabfile.factor_digest(d) == entry["digest"]
            print(json.dumps(dict(case=a.case, waves=i["waves"], workers=i["workers"], flags=flags, rep=rep, rc=rc, K=i["K"],
                                  ok=ok, launches=i["launches"], kernel_ms=round(i["kernel_ms"], 3), **counters(i))), flush=True)
            if not ok:
                nbad += 1
                if nbad == 1:
                    oracle_diff(entry, fix, d)
            if a.fresh:
                f.close()
                f = None
        if f is not None:
            f.close()
        print(json.dumps(dict(case=a.case, shape=shape, reps=a.reps, nbad=nbad)), flush=True)


def cmd_commits(a):
    for name in a.cases.split(","):
        entry, fix = load_case(name)
        for flags in ints(a.flags):
            f = handle(entry, fix, a.waves, a.workers, flags, a.lib)
            f.run(entry["kmax"], check=False)
            i0 = f.info()
            f.reset()
            rc = f.run(entry["kmax"], check=False)
            i = f.info()
            f.close()
            print(f"{name} flags {flags}: rc {rc} K {i['K']} workers {i['workers']} launches {i0['launches']}/{i['launches']} "
                  f"xcap {i0['xcap_digits']}/{i['xcap_digits']} short {i['short_commits']} by committer {i['committer_commits']} "
                  f"engine {i['engine_commits']}/{i['engine_sources']} farm jobs {i['farm_jobs']} items {i['farm_items']} "
                  f"kernel_ms {i0['kernel_ms']:.2f}/{i['kernel_ms']:.3f} = {1e3 * i['kernel_ms'] / max(i['K'], 1):.2f} us/col", flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = p.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("cases")
    r.add_argument("--workers", default="0")
    r.add_argument("--waves", default="0")
    r.add_argument("--flags", default="0")
    r.set_defaults(fn=cmd_run)
    r = sub.add_parser("repeat")
    r.add_argument("case")
    r.add_argument("--reps", type=int, default=3)
    r.add_argument("--shapes", default="0:0:0")
    r.add_argument("--fresh", action="store_true")
    r.set_defaults(fn=cmd_repeat)
    r = sub.add_parser("commits")
    r.add_argument("cases")
    r.add_argument("--workers", type=int, default=0)
    r.add_argument("--waves", type=int, default=0)
    r.add_argument("--flags", default="0,4,2")
    r.set_defaults(fn=cmd_commits)
    for r in sub.choices.values():
        r.add_argument("--lib", default=os.environ.get("SLIP_PROBE_LIB"))
    a = p.parse_args()
    a.fn(a)


if __name__ == "__main__":
    main()
