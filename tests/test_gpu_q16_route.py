"""GPU: the pairs route with q16 blocks in the on-demand ring (catalog.PAIR_BOUND_Q16, ABI 20).

_score_topk_pairs on 300 users x 3000 POIs (h up to 60, k = 50, PAIR_BLOCK_COLS = 512: five full
blocks and one of 440 columns), D = H = 64 and 32, three ways: q16 on, q16 off (hi words) and
PAIR_BOUNDED = False (the exact gather). ids and score bits are identical across the three, and
the plan events name the form. A model whose eta'_1 exceeds 2^-7 keeps the route it had (the
three-product table, hi words) whatever the knob says."""
import numpy as np
import pytest
import torch

from test_gpu_ondemand_refine import _model

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _run(m, data, k, q16, bounded=True):
    from poi_recommendation_models_amd import catalog
    from poi_recommendation_models_amd.catalog import DeviceCSR, _score_topk_pairs
    csr = DeviceCSR.from_arrays(data.indptr, data.indices, data.num_pois, DEV)
    old = catalog.PAIR_BOUNDED, catalog.PAIR_BOUND_Q16, catalog.PAIR_BLOCK_COLS
    catalog.PAIR_BOUNDED, catalog.PAIR_BOUND_Q16, catalog.PAIR_BLOCK_COLS = bounded, q16, 512
    try:
        ev = []
        ids, sc = _score_topk_pairs(m, csr, np.arange(data.num_users), k, None, None, None, None, force=True,
                                    events=ev)
    finally:
        catalog.PAIR_BOUNDED, catalog.PAIR_BOUND_Q16, catalog.PAIR_BLOCK_COLS = old
    torch.cuda.synchronize()
    plan = {kind: v for kind, e0, _, v in ev if e0 is None}
    stats = m._last_bound_stats.cpu().numpy() if bounded else None
    return ids.cpu().numpy(), sc.cpu().numpy().view(np.uint32), int(m._last_nan.item()), plan, stats


def _same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert a[2] == b[2]


@pytest.mark.parametrize("D,H", [(64, 64), (32, 32)])
def test_q16_route_equals_hi_word_and_exact_routes(D, H):
    from poi_recommendation_models_amd.synthetic import make_checkins
    data = make_checkins(300, 3000, 60, seed=13)
    m = _model(3000, D, H)
    on, off, exact = _run(m, data, 50, True), _run(m, data, 50, False), _run(m, data, 50, False, bounded=False)
    for r, words in ((on, "q16"), (off, "hi")):
        assert r[3]["pair_route"] == "ondemand" and r[3]["ondemand_products"] == 1, r[3]
        assert r[3]["ondemand_words"] == words and r[3]["block_cols"] == 512, r[3]
    assert exact[3]["pair_route"] == "exact" and "ondemand_words" not in exact[3]
    _same(on, exact)
    _same(on, off)
    # the last block has 440 columns (27 groups and 8 columns): were its ragged end read as zeros,
    # or any block's intervals not finite, those candidates would all be refined -- hundreds per
    # user. The q16 band of N is at most (1 + 2 x 128 (4g + eta2)) Qs ~ 2.5 Qs against the hi words'
    # 2 x 2^-7 A, with Qs <= A / 40 here (|m_s| averages over 40): within a factor 4 of each other.
    assert on[4][1] == 0 and off[4][1] == 0
    assert on[4][0] <= 4 * off[4][0], (on[4][0], off[4][0])
    print("D=%d H=%d refined per user: q16 %.1f (overflowed %d), hi words %.1f (overflowed %d)"
          % (D, H, on[4][0] / 300, on[4][1], off[4][0] / 300, off[4][1]))


def test_eta1_beyond_its_limit_keeps_its_route():
    from poi_recommendation_models_amd import catalog
    from poi_recommendation_models_amd.synthetic import make_checkins
    data = make_checkins(150, 2000, 60, seed=5)
    m = _model(2000, 64, 64, emb_std=0.42)
    eta1, eta3 = catalog.ondemand_widening(m, products=1)[1], catalog.ondemand_widening(m)[1]
    assert eta1 > catalog.PAIR_ONDEMAND_ETA1_MAX and eta3 <= catalog.PAIR_ONDEMAND_ETA_MAX, (eta1, eta3)
    on, off, exact = _run(m, data, 50, True), _run(m, data, 50, False), _run(m, data, 50, False, bounded=False)
    for r in (on, off):
        assert r[3]["pair_route"] == "ondemand" and r[3]["ondemand_products"] == 3, r[3]
        assert r[3]["ondemand_words"] == "hi", r[3]
    _same(on, exact)
    _same(on, off)
