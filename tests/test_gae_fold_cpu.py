"""CPU: what the chunked (two-level) GAE scan may differ from the sequential one by, stated in numpy before a GPU is involved.

csrc/gae.hip splits the time axis over waves and workgroups: every piece is reduced to an affine map A_in = Q + P * A_out in float64,
the maps are composed latest-first and every piece replays its rows from the composed carry-in.  That re-associates float64 products
and sums; after the float32 store it shows in about one element in 1e8.  tests/test_gae_gpu.py therefore allows the split forms
np.allclose(rtol=2e-7, atol=1e-7) and at most 1e-3 of an array's elements unequal (a wrong carry corrupts whole chunks).  The cap is
a condition on the INPUTS: here the reference arithmetic alone (helpers/gae_cases.py: chunked_scan, built from the oracle's own
float32 delta and coeff) must stay inside it on every input those tests use.  If a seed fails here, change the seed, not the cap."""
import numpy as np
import pytest

from helpers import gae_cases as G


def test_the_emulation_with_one_piece_is_the_oracle():
    """(C, W) = (1, 1) is the sequential scan: bit-equal to oracle.gae.dual_gae, i.e. delta, coeff and the head row ARE the oracle's."""
    for N in (70, 72):
        for p, pattern in G.CASES:
            arrs, params, o = G.form_case(N, p, pattern)
            got = G.chunked_scan(arrs, params, *G.chunkings(G.T_FORMS)["sequential"])
            for k in G.OUT_KEYS:
                assert np.array_equal(got[k], o[k]), (N, p, pattern, k)


@pytest.mark.parametrize("chunking", ["regsplit", "split3", "waves4", "waves16"])
@pytest.mark.parametrize("N", [70, 72])
@pytest.mark.parametrize("p,pattern", G.CASES)
def test_chunked_fold_stays_inside_the_gpu_tests_bounds(p, pattern, N, chunking):
    arrs, params, o = G.form_case(N, p, pattern)
    got = G.chunked_scan(arrs, params, *G.chunkings(G.T_FORMS)[chunking])
    for k in G.OUT_KEYS:
        assert np.isfinite(got[k]).all(), k
        assert np.allclose(got[k], o[k], rtol=2e-7, atol=1e-7), k
        assert (got[k] != o[k]).mean() <= 1e-3, (k, int((got[k] != o[k]).sum()))
        if params == (1.0, 1.0, 1.0, 1.0):
            # no decay: every coefficient is 0 or 1, the fold's products stay exact and only its sums re-associate: <= 1 float32 ulp
            ulp = np.abs(got[k].view(np.int32).astype(np.int64) - o[k].view(np.int32).astype(np.int64)).max()
            assert ulp <= 1, (k, int(ulp))


def test_the_cases_cover_what_they_claim():
    """the seams pattern has its ones exactly on the listed rows; the random patterns are near 0.3; all four parameters of set 0 differ."""
    assert len(set(G.PARAM_SETS[0])) == 4 and len(G.CASES) == 9
    arrs, _, _ = G.form_case(70, 0, "seams")
    assert sorted(np.flatnonzero(arrs["dones"].all(axis=1))) == sorted(G.SEAM_ROWS) and arrs["dones"].sum() == len(G.SEAM_ROWS) * 70
    arrs, _, _ = G.form_case(70, 0, "random")
    assert 0.27 < arrs["dones"].mean() < 0.33
    assert G.form_case(70, 0, "random_last_all")[0]["last_dones"].all() and not G.form_case(70, 0, "random_last_none")[0]["last_dones"].any()
    assert G.form_case(70, 0, "all")[0]["dones"].all() and not G.form_case(70, 0, "none")[0]["dones"].any()
