#!/usr/bin/env python3
"""The committer's phase times on the headline window (libslip_hip_cprof.so, `make cprof`: the committer's phase clock,
the workers do not stamp) as a small JSON for profiles/: bench.py's roofline.chain takes the committer's serial time per
column from the newest one.  The best of five runs; the phases, sub-steps and calibration of that run are printed too.
usage: commit_profile.py out.json [case] [workers] [waves]"""
import ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_case
import slip_lu_amd as sl
path = os.path.join(ROOT, "slip_lu_amd", "csrc", "libslip_hip_cprof.so")
name = sys.argv[2] if len(sys.argv) > 2 else "C4_n100k_c64"
workers = int(sys.argv[3]) if len(sys.argv) > 3 else 0
waves = int(sys.argv[4]) if len(sys.argv) > 4 else 0
entry, fix = load_case(name)
f = sl.Factorization(entry["n"], fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"], pivot=entry["pivot"], tol=entry["tol"],
                     limb_cap=entry["cap"], lib_path=path, workers=workers, waves=waves)
best = None
for rep in range(5):
    f.reset(); f.run(entry["kmax"], check=False)
    i = f.info()
    out = (C.c_ulonglong * 24)()
    f.lib.slip_hip_factor_phase_cycles(f.h, out)
    rec = (i["kernel_ms"], [int(out[q]) for q in range(24)], i)
    if best is None or rec[0] < best[0]:
        best = rec
f.close()
ms, o, i = best
cols = max(o[7], 1); us = lambda q: o[q] / 100.0
serial = sum(us(q) for q in (3, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19))
res = dict(case=name, kernel_ms=ms, columns=i["K"], committer_commits=i["committer_commits"], engine_commits=i["engine_commits"],
           batch_commits=i["batch_commits"], run_us=us(14),
           batches=o[6], committed_by_committer=o[7], rejects=o[8],
           us_total=dict(waiting_for_packages=us(0), packages_into_lds=us(1), rho_after_resync=us(2), serial=serial, publish_and_drain=us(4), verdicts=us(5)),
           serial_us_per_column=serial / cols, load_us_per_column=us(1) / cols, publish_us_per_column=(us(4) + us(5)) / cols,
           note="times of thread 0 of the committer workgroup (s_memrealtime, 10 ns ticks); each stamp costs about 0.05 us, ten per column")
json.dump(res, open(sys.argv[1], "w"), indent=1)
print(f"{name}: K {i['K']} kernel_ms {ms:.3f} by committer {i['committer_commits']} (run {i['batch_commits']}, engine {i['engine_commits']}, late sources {i['engine_sources']}); "
      f"batches {o[6]} columns {o[7]} rejects {o[8]} ready-at-poll {o[9]} retractions {i['retractions']} re-exports {i['reexports']}")
for q, nm in enumerate(["waiting for packages", "packages into LDS", "rho after a resync", "serial part (wave 0)", "publish + drain", "verdicts + frontier"]):
    print(f"    {nm:28s} {us(q):10.1f} us total  {us(q) / max(o[6], 1):8.2f} us per batch  {us(q) / cols:8.2f} us per column")
for q, nm in ((14, "run: side by side"), (10, "c: setup + intermed2"), (11, "c0: rows vs pivots"), (12, "c0: capacity"), (13, "c0: choose + diag"), (15, "c0: rho multiply"),
              (17, "c1: state + hash"), (18, "c1: late sources"), (19, "c1: finals + search + hand-back"), (16, "c: record + rings")):
    print(f"        {nm:34s} {us(q):10.1f} us total  {us(q) / cols:8.2f} us per column")
c0, c1, c2 = o[20], o[21], o[22]
if c0:
    print(f"    calibration in the committer: dependent LDS read {(c0 >> 32) / 256:.0f} cycles = {(c0 & 0xFFFFFFFF) * 10 / 256:.0f} ns; dependent VALU mul-add "
          f"{(c1 >> 32) / 1024:.1f} cycles = {(c1 & 0xFFFFFFFF) * 10 / 1024:.1f} ns; s_memrealtime stamp {c2 / 64:.0f} cycles; clock {(c1 >> 32) / max((c1 & 0xFFFFFFFF) * 10, 1):.2f} GHz")
print(json.dumps(res))
