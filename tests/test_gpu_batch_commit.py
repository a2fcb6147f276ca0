"""The committer's run (candidates-only columns of a batch committed side by side, ref_lu_pipe_commit.h) on the device:
the headline window and 10teams against their golden digests, the pivot-edge corpus, and the counter that says how many
columns went through the run."""
import pytest

import pivot_corpus as pc
from conftest import check_against_golden, load_case

pytestmark = pytest.mark.gpu


def _run(name, **kw):
    import slip_lu_amd as sl
    entry, fix = load_case(name)
    res = sl.factorize(entry["n"], fix["Ap"], fix["Ai"], fix["Alen"], fix["Alimbs"], fix["q"], pivot=entry["pivot"], tol=entry["tol"],
                       kmax=entry["kmax"], limb_cap=entry["cap"], **kw)
    check_against_golden(entry, fix, res)
    return res["info"]


def test_gpu_run_on_the_headline_window():
    i = _run("C4_n100k_c64")
    assert i["batch_commits"] > 0, i
    assert i["batch_commits"] <= i["committer_commits"] - i["engine_commits"], i
    print(f"C4 window: {i['batch_commits']} of {i['committer_commits']} committer commits through the run "
          f"({100.0 * i['batch_commits'] / max(i['committer_commits'], 1):.1f} %)")


def test_gpu_run_leaves_the_chain_engine_alone():
    i = _run("10teams")
    assert i["engine_commits"] > 0, i
    print(f"10teams: batch {i['batch_commits']} engine {i['engine_commits']} committer {i['committer_commits']}")


@pytest.mark.parametrize("kw", [{}, {"workers": 1}, {"waves": 2}], ids=["default", "workers1", "waves2"])
def test_gpu_run_on_pivot_corpus(kw):
    import slip_lu_amd as sl
    bad, batch, committer = [], 0, 0
    for run in pc.runs():
        n, Ap, Ai, Alen, Alimbs, q = pc.matrix(run["matrix"])
        res = sl.factorize(n, Ap, Ai, Alen, Alimbs, q, pivot=run["pivot"], tol=run["tol"], check=False, **kw)
        batch += res["info"]["batch_commits"]
        committer += res["info"]["committer_commits"]
        try:
            pc.check_run(run, res)
        except AssertionError as e:
            bad.append((pc.label(run), str(e)[:80]))
    print(f"pivot corpus {kw}: {batch} of {committer} committer commits through the run")
    assert not bad, "%d of %d runs differ from the reference: %s" % (len(bad), len(pc.runs()), bad[:8])
