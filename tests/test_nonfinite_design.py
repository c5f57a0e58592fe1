"""CPU: the designed overflow / underflow model of tests/_nonfinite.py is what the GPU tests
(tests/test_gpu_nonfinite.py) take it for.

* Every (history item, candidate) attention logit of every shape, in float64 from the parameters,
  is ordinary (|a| <= 40) or far beyond a threshold (a >= 150: e = inf; a <= -150: e = 0), so no
  arithmetic -- fp32, fp16x6, fp16x3, the 3-product bound -- can disagree about WHICH pairs are
  non-finite; every |h . t| is below 1e3, so no finite e * s overflows.
* The numpy oracle's NaN set of every user is exactly the designed one.
* The product-overflow band: where e_j is finite and e_j |h_j . t| is not, the oracle (the
  reference's order: each term divided by S^beta first) stays finite and the pair-factorised
  N / S^beta is inf - inf = NaN once two such terms have opposite signs; its limits are measured.
* The top-k comparison helper rejects a NaN prefix in the wrong order and a NaN candidate swapped
  for the best finite one (as test_torch_pairs_checker.py shows for its checker)."""
import numpy as np
import pytest

import _nonfinite as nf
from oracle import nais_oracle

# (variant, D, H) of test_gpu_nonfinite.py
SHAPES = [("basic", 32, 32), ("basic", 64, 64), ("basic", 100, 40), ("basic", 192, 192),
          ("basic", 128, 128), ("region_distance", 64, 64)]
K = 50


@pytest.mark.parametrize("variant,D,H", SHAPES)
def test_design_logits_are_far_from_the_thresholds_and_nan_sets_are_the_designed_ones(variant, D, H):
    d = nf.build(D=D, H=H, variant=variant)
    assert d.P == 1300 and d.P - 1 in d.ovf_c[0]                       # the last column is designed
    blocks = lambda c: set((np.asarray(c) // 512).tolist())            # noqa: E731
    for cs in (*d.ovf_c, d.und_c):
        assert blocks(cs) == {0, 1, 2}                                 # first, interior, last block
    assert len(d.ovf_c[0]) < K < len(d.ovf_c[1])
    assert d.masked_c in d.ovf_c[0] and d.masked_c in d.history("masked")
    items = np.unique(np.concatenate([h for _, h in d.users]))
    a, s = nf.pair_values64(d, items)
    row = {int(it): i for i, it in enumerate(items)}
    far = (np.abs(a) <= 40) | (a >= 150) | (a <= -150)
    assert far.all(), a[~far][:8]
    assert np.abs(s).max() < 1e3
    nan_total = 0
    for name, hist in d.users:
        want = d.designed_nan(hist)
        cand, ref = nf.oracle_scores(d, hist)
        got = np.zeros(d.P, dtype=bool)
        got[cand[np.isnan(ref)]] = True
        assert np.array_equal(got, want), (name, np.nonzero(got != want)[0][:10])
        # the designed set restated from the float64 logits: some e = inf, or every e = 0
        if len(hist):
            ah = a[[row[int(j)] for j in hist]]
            by_logit = (ah >= 150).any(0) | (ah <= -150).all(0)
            by_logit[hist] = False
            assert np.array_equal(by_logit, want), name
        nan_total += int(want.sum())
        fin = ref[~np.isnan(ref)]
        assert np.isfinite(fin).all() and fin.min() >= 0.0 and fin.max() <= 1.0
        ids, sc = nais_oracle.topk_ids(cand, ref, K)
        n = int(np.isnan(sc).sum())
        assert n == min(K, int(want.sum())) and np.isnan(sc[:n]).all()
        assert np.array_equal(ids[:n], np.nonzero(want)[0][:n])        # NaN first, ids ascending
    sizes = {n: int(d.designed_nan(h).sum()) for n, h in d.users}
    assert sizes == {"plain": 0, "ovf_small": 19, "ovf_big": 90, "ovf_two": 109, "und_mixed": 0,
                     "und_only": 120, "und_single": 120, "both": 19, "empty": 0, "long": 109,
                     "masked": 18, "ovf_single": 90}, sizes
    assert nan_total == sum(sizes.values())


def test_long_history_places_the_overflowing_items_past_64_and_128():
    d = nf.build()
    h = d.history("long")
    assert len(h) == 150
    assert 64 <= list(h).index(d.ovf_h[0]) < 128 <= list(h).index(d.ovf_h[1])


LN_FLT_MAX = float(np.log(np.finfo(np.float32).max))    # 88.7228


@pytest.mark.parametrize("band_a", [83.0, 84.0, 84.6, 85.0, 87.0, 88.5, 89.0])
def test_product_overflow_band_oracle_and_factorised_form(band_a):
    """Items A (s = a) and B (s = a - 300) on the 86 designed candidates, users A, B and A + B.
    Inside the band -- e finite (a < ln FLT_MAX = 88.72) and both e |s| above FLT_MAX
    (a > 88.72 - ln|s|, 84.26 at a = 87) -- the oracle gives 1.0, 0.0 and 0.0 (0.5 once the sum of the
    two e overflows too, a > 88.03: every term is then e / inf = 0), the factorised form 1.0, 0.0
    and NaN. Below the band both forms agree and are finite; above it e = inf and both
    are NaN."""
    d = nf.build(band_a=band_a)
    a, s = nf.pair_values64(d, np.array(d.band_h))
    a, s = a[:, d.band_c], s[:, d.band_c]
    assert np.abs(a - band_a).max() < 0.2                                  # the other units add ~0.01
    assert np.abs(s[0] - band_a).max() < 0.2 and np.abs(s[1] - (band_a - 300)).max() < 0.2
    lo = LN_FLT_MAX - np.log(np.abs(s)).min()       # both products overflow above this a
    assert abs(lo - (LN_FLT_MAX - np.log(band_a))) < 0.01
    assert abs(a - lo).min() > 0.2 and abs(a - LN_FLT_MAX).min() > 0.2     # not on a limit
    inside, above = lo < band_a < LN_FLT_MAX, band_a > LN_FLT_MAX
    res = {}
    for name, hist in d.users:
        cand, ref = nf.oracle_scores(d, hist)
        cand2, fac = nf.factorised_scores(d, hist)
        assert np.array_equal(cand, cand2)
        on = np.isin(cand, d.band_c)
        # off the designed candidates the two forms are the same ordinary numbers
        assert np.isfinite(ref[~on]).all() and np.abs(ref[~on] - fac[~on]).max() <= 1e-6
        res[name] = (ref[on], fac[on])
    if above:
        for name in res:
            assert np.isnan(res[name][0]).all() and np.isnan(res[name][1]).all(), name
        return
    for name, want in (("A", 1.0), ("B", 0.0)):
        assert np.all(res[name][0] == want) and np.all(res[name][1] == want), name
    ref, fac = res["AB"]
    # finite either way: 5.5e18 * 87 - 5.5e18 * 213 < 0, or, once S = 2 e overflows as well
    # (a > 88.72 - ln 2 = 88.03), every term e / inf = 0 and the logit 0
    assert abs(band_a - (LN_FLT_MAX - np.log(2.0))) > 0.2
    assert np.all(ref == (0.5 if band_a > LN_FLT_MAX - np.log(2.0) else 0.0)), ref
    if inside:
        assert np.isnan(fac).all()                   # inf - inf
    else:
        assert np.all(fac == 0.0)


def _lists():
    d = nf.build()
    out = {}
    for name in ("ovf_small", "ovf_big"):
        cand, ref = nf.oracle_scores(d, d.history(name))
        ids, sc = nais_oracle.topk_ids(cand, ref, K)
        out[name] = (cand, ref, ids, sc, dict(zip(cand.tolist(), ref.tolist())))
    return out


def test_topk_helper_accepts_the_oracle_and_rejects_wrong_nan_rankings():
    for name, (cand, ref, ids, sc, lut) in _lists().items():
        n = nf.assert_topk_matches(ids, sc, ids.copy(), sc.copy(), lut)
        assert n == (19 if name == "ovf_small" else K)
        # (1) the NaN prefix sorted descending by id
        bad = ids.copy()
        bad[:n] = bad[:n][::-1]
        with pytest.raises(AssertionError):
            nf.assert_topk_matches(ids, sc, bad, sc, lut)
        # (2) one NaN candidate replaced by the best finite one not yet listed
        fin = ~np.isnan(ref) & ~np.isin(cand, ids)
        best = int(cand[fin][np.argmax(ref[fin])])
        bad, bsc = ids.copy(), sc.copy()
        bad[n - 1], bsc[n - 1] = best, lut[best]
        with pytest.raises(AssertionError):
            nf.assert_topk_matches(ids, sc, bad, bsc, lut)
        # ... also when it keeps a NaN score there (a key built from the wrong id)
        bsc[n - 1] = np.nan
        with pytest.raises(AssertionError):
            nf.assert_topk_matches(ids, sc, bad, bsc, lut)
        # (3) a NaN candidate ranked behind the finite ones
        if n < K:
            order = np.r_[np.arange(1, K), 0]
            with pytest.raises(AssertionError):
                nf.assert_topk_matches(ids, sc, ids[order], sc[order], lut)
