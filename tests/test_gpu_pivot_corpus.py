"""The pivot-edge corpus (tests/pivot_corpus.py) on the device: every run of the compiled reference, bit-exact, under
the default launch, one worker, two waves, and with the chain engine off (no full packages)."""
import pytest

import pivot_corpus as pc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kw", [{}, {"workers": 1}, {"waves": 2}, {"debug_flags": 8}], ids=["default", "workers1", "waves2", "engine_off"])
def test_gpu_matches_reference_on_pivot_corpus(kw):
    import slip_lu_amd as sl
    bad = []
    for run in pc.runs():
        n, Ap, Ai, Alen, Alimbs, q = pc.matrix(run["matrix"])
        res = sl.factorize(n, Ap, Ai, Alen, Alimbs, q, pivot=run["pivot"], tol=run["tol"], check=False, **kw)
        try:
            pc.check_run(run, res)
        except AssertionError as e:
            bad.append((pc.label(run), str(e)[:80]))
    assert not bad, "%d of %d runs differ from the reference: %s" % (len(bad), len(pc.runs()), bad[:8])
