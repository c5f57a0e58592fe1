"""GPU: the bound table with one f16 product per attention-logit term (include/nais.h
nais_pair_table_bound1_queued, ABI 17; catalog_score_x3b_kernel<..., ONE = true>; DESIGN.md (d),
"One product per logit term").

1. Table words. For every pair of small tables, e^ and the truncated e*s read from the new entry's
   hi word bound the fp16x6 pair values (e6, e6 s6 of nais_pair_recompute) under the one-product
   widening: e6 in [e^ (1 - eta'), e^ (1 + 2^-7)(1 + eta')] and |e6 s6 - es~| within the per-term
   radius of nais_pairs.hip make_bounds. 1, 31, 33, 129 and 300 items (the 32-row chunk and
   128-row group edges), three column blocks of a catalog whose size is no multiple of 32 (the last
   tile's lanes clamp to row P - 1), items that are also candidates (the self-pair mask: word 0),
   D / H of 32 / 32, 64 / 64 and 40 / 40 (padded). The queued and fixed-grid tables are equal word
   for word. The largest observed share of eta' is printed.
2. The whole route: ids and score bits of the default (one-product) job equal the exact route's
   and the three-product form's, k = 50 and k = 1, and on a column shard; the plan events name the
   form. The non-finite model of tests/_nonfinite.py is refused by the gate and takes split16; a
   model whose eta'_1 exceeds 2^-7 while eta'_3 stays within 2^-9 takes the three-product form."""
import numpy as np
import pytest
import torch

from test_gpu_ondemand_refine import _model, _recompute, _scales

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
P_T, W_T = 1301, 512      # blocks of 512, 512 and 277 columns; 1301 = 40 * 32 + 21


def _bound1(m, items, c0, w, work):
    from poi_recommendation_models_amd import _capi
    J = len(items)
    hi = torch.full((J, W_T), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    _capi.check(_capi.load().nais_pair_table_bound1_queued(
        m._score_params(), items.data_ptr(), J, c0, w, None, None, None, hi.data_ptr(), W_T,
        None if work is None else work.data_ptr(), None), "nais_pair_table_bound1_queued")
    torch.cuda.synchronize()
    return hi.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("D,H", [(32, 32), (64, 64), (40, 40)])
def test_one_product_hi_words_bound_the_fp16x6_values(D, H):
    from poi_recommendation_models_amd import catalog
    m = _model(P_T, D, H, emb_std=0.3)
    _, eta, ds = catalog.ondemand_widening(m, products=1)
    assert np.isfinite(eta) and eta <= catalog.PAIR_ONDEMAND_ETA1_MAX, eta    # the interval the gather applies
    eta2 = 1.02 * eta + 2.0 ** -21
    work = torch.zeros(1, dtype=torch.int32, device=DEV)
    tiny = 2.0 ** -126
    share = 0.0
    for J in (1, 31, 33, 129, 300):
        # POIs 5 .. 4 + J lie in the first column block: item == candidate pairs occur there
        items = torch.arange(5, 5 + J, dtype=torch.int64, device=DEV)
        for c0 in (0, W_T, 2 * W_T):
            w = min(W_T, P_T - c0)
            hw = _bound1(m, items, c0, w, None)
            assert np.all(hw[:, w:] == 0x5A5A5A5A)                  # nothing past the block
            work.fill_(777)                                          # the launch zeroes it
            np.testing.assert_array_equal(_bound1(m, items, c0, w, work), hw, err_msg=f"J={J} c0={c0}")
            hw = hw[:, :w]
            rowsc, colsc = _scales(m, items, c0, w, W_T)
            e6, es6 = (t.astype(np.float64) for t in
                       _recompute(m, items, rowsc, colsc, c0, w, np.arange(J), c0 + np.arange(w)))
            eh = (hw << 16).view(np.float32).astype(np.float64)      # e^: e~ truncated to 16 bits
            esw = hw.view(np.float32).astype(np.float64)             # es~: the word as the gather reads it
            if c0 == 0:   # the self pairs: e = +0 in both arithmetics, e * s = +-0 (the sign of s)
                jj = np.arange(J)
                assert not (hw[jj, 5 + jj] & 0x7FFFFFFF).any() and not e6[jj, 5 + jj].any()
            assert np.all(e6 >= eh * (1 - eta) - tiny), (J, c0)
            assert np.all(e6 <= eh * (1 + 2.0 ** -7) * (1 + eta) + tiny), (J, c0)
            radius = (2.0 ** -7 + eta2) * np.abs(esw) + eh * (1 + 2.0 ** -7) * (1 + eta) * ds + tiny
            assert np.all(np.abs(es6 - esw) <= radius), (J, c0)
            ok = eh > 2.0 ** -100
            r = e6[ok] / eh[ok]        # in [1, 1 + 2^-7) were the arithmetics equal: what eta' has to cover
            share = max(share, float(np.max(1.0 - r)) / eta, float(np.max(r / (1 + 2.0 ** -7) - 1.0)) / eta)
    print("D=%d H=%d eta'_1=%.3e delta_s=%.3e largest observed share of eta' used: %.2e" % (D, H, eta, ds, share))
    assert share <= 1.0


def _run(m, data, k, form, users=None, cols=None):
    """form: 1 / 3 = the on-demand route with the one- / three-product knob, "exact" = the exact
    gather. Returns (ids, score bits, NaN count, events as a dict of the plan's scalar entries)."""
    from poi_recommendation_models_amd import catalog
    from poi_recommendation_models_amd.catalog import DeviceCSR, _score_topk_pairs
    csr = DeviceCSR.from_arrays(data.indptr, data.indices, data.num_pois, DEV)
    users = np.arange(data.num_users) if users is None else users
    old = catalog.PAIR_BOUNDED, catalog.PAIR_ONDEMAND_REFINE, catalog.PAIR_ONDEMAND_ONE_PRODUCT
    catalog.PAIR_BOUNDED, catalog.PAIR_ONDEMAND_REFINE = form != "exact", True
    catalog.PAIR_ONDEMAND_ONE_PRODUCT = form == 1
    try:
        ev = []
        ids, sc = _score_topk_pairs(m, csr, users, k, None, None, None, None, force=True, cols=cols, events=ev)
    finally:
        catalog.PAIR_BOUNDED, catalog.PAIR_ONDEMAND_REFINE, catalog.PAIR_ONDEMAND_ONE_PRODUCT = old
    torch.cuda.synchronize()
    plan = {kind: v for kind, e0, _, v in ev if e0 is None}
    return ids.cpu().numpy(), sc.cpu().numpy().view(np.uint32), int(m._last_nan.item()), plan


def _same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert a[2] == b[2]


@pytest.mark.parametrize("D,H", [(64, 64), (40, 40)])
def test_one_product_route_equals_exact_and_three_product_routes(D, H):
    from poi_recommendation_models_amd.synthetic import make_checkins
    data = make_checkins(300, 4000, 200, seed=13)
    lens = np.diff(data.indptr)
    assert lens.min() >= 1 and lens.max() > 150, (lens.min(), lens.max())
    m = _model(4000, D, H)
    for k, cols in ((50, None), (1, None), (50, (777, 3001))):
        one, three, exact = (_run(m, data, k, f, cols=cols) for f in (1, 3, "exact"))
        assert one[3]["pair_route"] == "ondemand" and one[3]["ondemand_products"] == 1, one[3]
        assert three[3]["pair_route"] == "ondemand" and three[3]["ondemand_products"] == 3, three[3]
        assert exact[3]["pair_route"] == "exact"
        assert 2.0 ** -9 < one[3]["ondemand_eta1"] <= 2.0 ** -7 and one[3]["ondemand_eta"] <= 2.0 ** -9
        _same(one, exact)
        _same(one, three)
    st = m._last_bound_stats.cpu().numpy()
    print("D=%d H=%d refined per user (last job)" % (D, H), st[0] / 300, "overflowed", st[1])


def test_nonfinite_model_is_refused_and_takes_split16():
    import _nonfinite as nf
    from poi_recommendation_models_amd import catalog
    from poi_recommendation_models_amd.catalog import DeviceCSR
    from test_gpu_parity import _model as parity_model
    d = nf.build(D=32, H=32)
    m = parity_model("basic", d.params, precision="fp16x6")
    for products in (1, 3):
        eta = catalog.ondemand_widening(m, products=products)[1]
        assert not np.isfinite(eta) or eta > (catalog.PAIR_ONDEMAND_ETA1_MAX if products == 1
                                              else catalog.PAIR_ONDEMAND_ETA_MAX), (products, eta)
    indptr, indices = d.csr_arrays()
    data = type("D", (), dict(indptr=indptr, indices=indices, num_pois=d.P, num_users=len(d.users)))
    users = np.array([i for i, (n, h) in enumerate(d.users) if len(h)])
    default, exact = _run(m, data, 20, 1, users=users), _run(m, data, 20, "exact", users=users)
    assert default[3]["pair_route"] == "split16" and default[3]["ondemand_products"] == 0, default[3]
    assert default[3]["ondemand_eta_accepted"] is False
    np.testing.assert_array_equal(default[0], exact[0])
    nan = np.isnan(default[1].view(np.float32))
    np.testing.assert_array_equal(nan, np.isnan(exact[1].view(np.float32)))
    np.testing.assert_array_equal(default[1][~nan], exact[1][~nan])
    assert default[2] == exact[2]


def test_eta1_beyond_its_limit_takes_the_three_product_form():
    """An embedding scale at which eta'_1 > 2^-7 while eta'_3 <= 2^-9: the default route runs the
    three-product table, says so, and returns the exact route's lists."""
    from poi_recommendation_models_amd import catalog
    from poi_recommendation_models_amd.synthetic import make_checkins
    data = make_checkins(150, 2000, 60, seed=5)
    m = _model(2000, 64, 64, emb_std=0.42)
    eta1, eta3 = catalog.ondemand_widening(m, products=1)[1], catalog.ondemand_widening(m)[1]
    assert eta1 > catalog.PAIR_ONDEMAND_ETA1_MAX and eta3 <= catalog.PAIR_ONDEMAND_ETA_MAX, (eta1, eta3)
    default, exact = _run(m, data, 50, 1), _run(m, data, 50, "exact")
    assert default[3]["pair_route"] == "ondemand" and default[3]["ondemand_products"] == 3, default[3]
    assert default[3]["ondemand_eta1"] == eta1 and default[3]["ondemand_eta"] == eta3
    _same(default, exact)
