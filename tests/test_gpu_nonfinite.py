"""GPU: catalog scoring, top-k and the forward against the numpy oracle where exp overflows or
underflows by arithmetic (no max-subtraction; inf / inf and 0 / 0 give
NaN exactly as in the reference), on the designed model of tests/_nonfinite.py -- rows in which
SOME candidates are NaN and the rest are finite, which is what a saturating model produces and
where the bounded route's pruning meets NaN keys. tests/test_nonfinite_design.py shows on the CPU
that the NaN sets are the designed ones and that no logit lies within 40 of a threshold.

* score rows: the NaN mask, the -1 history columns (one of them a designed candidate), the finite
  scores and the NaN count (the "counted above, but not a candidate" decrement) of both catalog
  strategies, on the tuned, padded and generic-shape kernels;
* top-k: the NaN prefix (ascending ids, NaN ranks above +inf) and the finite remainder of the
  direct route and of the exact, split16 and default pair routes; the pair routes bit-identical;
  the ondemand gate refuses the model; a 64-key survivor list (mostly-NaN users overflow it) and a
  column shard whose ends cut a designed candidate set;
* forward(): overflow, 0 / 0 and masked (inf * 0) rows;
* the product-overflow band: e_j finite, e_j |h_j . t| not. Every route returns the
  pair-factorised form's values there, which is the reference's 1.0 / 0.0 for one such item and
  NaN (reference: 0.0) for two of opposite sign. (These cases found the per-user and forward
  kernels fusing e * s into the running sum: 1.0 where the pair routes gave NaN; nais_kernels.hip
  mul_rn now rounds the product on its own, as the tables do.)"""
import functools

import numpy as np
import pytest
import torch

import _nonfinite as nf
from _helpers import SCORE_ATOL
from oracle import nais_oracle
from test_gpu_parity import _model, _t

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
K = 50

SHAPES = [("basic", "fp32", 32, 32), ("basic", "fp16x6", 32, 32), ("basic", "fp16x3", 32, 32),
          ("basic", "fp16x6", 64, 64), ("basic", "fp16x6", 100, 40), ("basic", "fp16x6", 192, 192),
          ("basic", "fp16x6", 128, 128), ("region_distance", "fp16x6", 64, 64)]


@functools.lru_cache(maxsize=None)
def _ref(variant, D, H):
    """The designed model and every user's (candidates, oracle scores), computed once per shape
    and shared read-only."""
    d = nf.build(D=D, H=H, variant=variant)
    refs = []
    for _, hist in d.users:
        cand, ref = nf.oracle_scores(d, hist)
        cand.setflags(write=False)
        ref.setflags(write=False)
        refs.append((cand, ref))
    return d, refs


@functools.lru_cache(maxsize=None)
def _band_ref(D, H):
    """The band model at a = 87: users A and B as the oracle has them, A + B as the factorised
    restatement has it (test_nonfinite_design.py: 1.0, 0.0 and NaN on the designed candidates)."""
    d = nf.build(D=D, H=H, band_a=87.0)
    refs = []
    for name, hist in d.users:
        cand, ref = nf.factorised_scores(d, hist) if name == "AB" else nf.oracle_scores(d, hist)
        on = np.isin(cand, d.band_c)
        want = {"A": 1.0, "B": 0.0}.get(name)
        assert np.isnan(ref[on]).all() if want is None else np.all(ref[on] == want)
        assert np.isfinite(ref[~on]).all()
        refs.append((cand, ref))
    return d, refs


def _csr(d):
    from poi_recommendation_models_amd.catalog import DeviceCSR
    return DeviceCSR.from_arrays(*d.csr_arrays(), d.P, DEV)


def _check_rows(d, refs, rows, last_nan, tag):
    total = 0
    for u, (name, hist) in enumerate(d.users):
        cand, ref = refs[u]
        assert np.all(rows[u][hist] == -1.0), (tag, name)          # history columns, designed or not
        got = rows[u][cand]
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (
            tag, name, cand[np.isnan(got) != np.isnan(ref)][:10].tolist())
        ok = ~np.isnan(ref)
        assert np.max(np.abs(got[ok] - ref[ok])) <= SCORE_ATOL, (tag, name, np.max(np.abs(got[ok] - ref[ok])))
        total += int(np.isnan(ref).sum())
    assert last_nan == total, (tag, last_nan, total)
    return total


@pytest.mark.parametrize("strategy", ["direct", "pairs"])
@pytest.mark.parametrize("variant,precision,D,H", SHAPES)
def test_score_rows_vs_oracle(variant, precision, D, H, strategy):
    from poi_recommendation_models_amd.catalog import score_catalog
    d, refs = _ref(variant, D, H)
    m = _model(variant, d.params, precision=precision)
    rows = score_catalog(m, _csr(d), range(len(d.users)), strategy=strategy, **d.side()).cpu().numpy()
    total = _check_rows(d, refs, rows, int(m._last_nan.item()), (variant, precision, D, H, strategy))
    print(variant, precision, D, H, strategy, "NaN candidates compared:", total)


def _pairs(m, d, k, route, cols=None, surv_cap=None):
    """route: "exact" (PAIR_BOUNDED off), "split16" (PAIR_ONDEMAND_REFINE off) or "default"."""
    from poi_recommendation_models_amd import catalog
    old = catalog.PAIR_BOUNDED, catalog.PAIR_ONDEMAND_REFINE, catalog.PAIR_SURV_CAP
    if route == "exact":
        catalog.PAIR_BOUNDED = False
    elif route == "split16":
        catalog.PAIR_ONDEMAND_REFINE = False
    if surv_cap is not None:
        catalog.PAIR_SURV_CAP = surv_cap
    try:
        ev = []
        ids, sc = catalog._score_topk_pairs(m, _csr(d), np.arange(len(d.users)), k, d.region_of, d.coords,
                                            None, None, force=True, cols=cols, events=ev)
        torch.cuda.synchronize()
        stats = m._last_bound_stats.cpu().numpy() if route != "exact" else None
    finally:
        catalog.PAIR_BOUNDED, catalog.PAIR_ONDEMAND_REFINE, catalog.PAIR_SURV_CAP = old
    took = [v for kind, _, _, v in ev if kind == "pair_route"]
    return ids.cpu().numpy(), sc.cpu().numpy(), int(m._last_nan.item()), took, stats


def _topk_refs(d, refs, k, cols=None):
    out = []
    for cand, ref in refs:
        if cols is not None:
            keep = (cand >= cols[0]) & (cand < cols[1])
            cand, ref = cand[keep], ref[keep]
        ids, sc = nais_oracle.topk_ids(cand, ref, k)
        out.append((ids, sc, dict(zip(cand.tolist(), ref.tolist())), int(np.isnan(ref).sum())))
    return out


def _check_lists(d, want, ids, sc, last_nan, tag):
    """Every user's list against the oracle's; returns the NaN entries compared."""
    seen = 0
    for u, (name, _) in enumerate(d.users):
        rid, rsc, lut, _ = want[u]
        try:
            seen += nf.assert_topk_matches(rid, rsc, ids[u], sc[u], lut)
        except AssertionError as e:
            raise AssertionError(f"{tag} user {name}: {e}") from e
    total = sum(w[3] for w in want)
    assert last_nan == total, (tag, last_nan, total)       # every NaN candidate, listed or not
    return seen


def _same_lists(a, b, tag):
    np.testing.assert_array_equal(a[0], b[0], err_msg=str(tag))
    nan = np.isnan(a[1])
    np.testing.assert_array_equal(nan, np.isnan(b[1]), err_msg=str(tag))              # positions
    np.testing.assert_array_equal(a[1].view(np.uint32)[~nan], b[1].view(np.uint32)[~nan], err_msg=str(tag))
    assert a[2] == b[2], (tag, a[2], b[2])


def _all_routes(d, refs, m, k, tag, cols=None, surv_cap=None, direct=True):
    from poi_recommendation_models_amd.catalog import score_topk
    want = _topk_refs(d, refs, k, cols)
    if direct:
        ids, sc = score_topk(m, _csr(d), range(len(d.users)), k, strategy="direct", **d.side())
        n = _check_lists(d, want, ids.cpu().numpy(), sc.cpu().numpy(), int(m._last_nan.item()), (tag, "direct"))
        print(tag, "direct: NaN entries compared", n)
    got = {r: _pairs(m, d, k, r, cols=cols, surv_cap=surv_cap) for r in ("exact", "split16", "default")}
    # a saturating model stays off the ondemand route: its proven |a| bound is what lets that
    # route ignore non-finite sums
    assert [got[r][3] for r in ("exact", "split16", "default")] == [["exact"], ["split16"], ["split16"]], \
        [got[r][3] for r in got]
    for r, g in got.items():
        n = _check_lists(d, want, g[0], g[1], g[2], (tag, r))
        if g[4] is not None:
            print(tag, r, "NaN entries compared", n, "refined per user", g[4][0] / len(d.users),
                  "overflowed users", int(g[4][1]))
        else:
            print(tag, r, "NaN entries compared", n)
    _same_lists(got["split16"], got["exact"], (tag, "split16 vs exact"))
    _same_lists(got["default"], got["exact"], (tag, "default vs exact"))
    return got


def _assert_gate_refuses(m):
    from poi_recommendation_models_amd import catalog
    eta = catalog.ondemand_widening(m)[1]
    assert not np.isfinite(eta) or eta > catalog.PAIR_ONDEMAND_ETA_MAX, eta


@pytest.mark.parametrize("variant,precision,D,H,k", [(*s, K) for s in SHAPES] + [("basic", "fp16x6", 32, 32, 1)])
def test_topk_vs_oracle_on_every_route(variant, precision, D, H, k):
    d, refs = _ref(variant, D, H)
    m = _model(variant, d.params, precision=precision)
    if variant == "basic":
        _assert_gate_refuses(m)
    _all_routes(d, refs, m, k, (variant, precision, D, H, k))
    if k == K:   # the designed rows are what the lists show
        ids, sc = nais_oracle.topk_ids(*refs[d.names.index("ovf_small")], k)
        assert int(np.isnan(sc).sum()) == 19 and np.isfinite(sc[19:]).all()
        assert np.isnan(nais_oracle.topk_ids(*refs[d.names.index("ovf_big")], k)[1]).all()


@pytest.mark.parametrize("D,H", [(32, 32), (64, 64)])
def test_topk_small_survivor_list_overflows_on_nan_users(D, H):
    """64 survivor keys: a user with 90 or more NaN candidates (upper key 0xFFFFFFFF each) cannot
    keep them and takes the refine-every-column path, with the same lists."""
    d, refs = _ref("basic", D, H)
    m = _model("basic", d.params, precision="fp16x6")
    got = _all_routes(d, refs, m, K, ("surv_cap 64", D, H), surv_cap=64, direct=False)
    assert got["split16"][4][1] > 0 and got["default"][4][1] > 0, "no user overflowed"


@pytest.mark.parametrize("cols", [(300, 1111), (1111, 1300)])
def test_topk_column_shard_cuts_a_designed_set(cols):
    """Shard ends inside OVF_C_BIG (290..319, 1095..1124); the second shard ends at the last,
    designed column."""
    d, refs = _ref("basic", 64, 64)
    assert 290 < cols[0] < 319 or 1095 < cols[0] < 1124
    m = _model("basic", d.params, precision="fp16x6")
    _all_routes(d, refs, m, K, ("cols", cols), cols=cols, direct=False)


@pytest.mark.parametrize("D,H", [(32, 32), (64, 64)])
def test_forward_vs_oracle(D, H):
    d, _ = _ref("basic", D, H)
    m = _model("basic", d.params)
    A, B = d.ovf_h
    small, big = d.ovf_c
    pool = d.plain_pool
    rng = np.random.default_rng(D)
    plain = lambda n: rng.choice(pool, n, replace=False)      # noqa: E731
    rows = []       # (history of 13, target)
    for t in (small[0], small[7], d.P - 1):
        rows.append((np.r_[plain(12), A], t))                 # overflow: inf / inf
    for t in (big[0], big[-1]):
        rows.append((np.r_[plain(5), B, plain(7)], t))
    rows.append((np.r_[plain(11), A, B], big[40]))            # both items, one overflows
    rows.append((np.r_[plain(12), A], big[3]))                # the cross pair: finite, score ~0
    rows.append((np.r_[plain(12), B], small[2]))
    rows.append((np.r_[plain(12), A], A))                     # the masked pair overflows: inf * 0
    h = plain(13)
    rows.append((h, h[4]))                                    # an ordinary masked term
    rows.append((np.r_[plain(12), A], plain(1)[0]))           # overflowing item, ordinary target
    rows.append((np.r_[plain(12), d.und_h[0]], d.und_c[0]))   # one underflowing term of 13: finite
    rows.append((np.resize(np.array(d.und_h), 13), d.und_c[5]))   # every term underflows: 0 / 0
    for _ in range(3):
        rows.append((plain(13), plain(1)[0]))                 # ordinary
    hist = np.array([r[0] for r in rows], dtype=np.int64)
    tgt = np.array([r[1] for r in rows], dtype=np.int64)
    calls = [(hist, tgt)]
    U = np.array(d.und_h)                                     # underflow-only histories of 3 and 1
    calls.append((np.tile(U, (4, 1)), np.array([d.und_c[1], d.und_c[-1], small[0], pool[0]])))
    calls.append((np.array([[U[1]], [U[1]], [B], [B]]), np.array([d.und_c[60], pool[1], big[50], small[1]])))
    seen = 0
    for hist, tgt in calls:
        ref, nan = nais_oracle.forward_basic(d.params, hist, tgt)
        got = m(_t(hist), _t(tgt)).cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (np.isnan(got), np.isnan(ref))
        assert int(m._last_nan.item()) == nan
        ok = ~np.isnan(ref)
        assert np.max(np.abs(got[ok] - ref[ok])) <= SCORE_ATOL
        seen += nan
    assert seen == 6 + 1 + 1 + 2 + 2       # overflow rows, inf * 0, 0 / 0 of 13, 0 / 0 of 3, of 1 (0 / 0, inf / inf)
    print("forward", D, H, "NaN rows compared:", seen)


BAND_SHAPES = [("fp32", 32, 32), ("fp16x6", 32, 32), ("fp16x3", 32, 32), ("fp16x6", 64, 64),
               ("fp16x6", 100, 40), ("fp16x6", 192, 192)]


@pytest.mark.parametrize("strategy", ["direct", "pairs"])
@pytest.mark.parametrize("precision,D,H", BAND_SHAPES)
def test_product_overflow_band_score_rows(precision, D, H, strategy):
    """a = 87 on the designed candidates: e = 6e37 is finite, e * 87 and e * (-213) are not. Users
    A and B match the oracle (1.0 / 0.0); user A + B is inf - inf = NaN in the pair-factorised
    form (the oracle: 0.0), counted -- the documented behaviour."""
    from poi_recommendation_models_amd.catalog import score_catalog
    d, refs = _band_ref(D, H)
    m = _model("basic", d.params, precision=precision)
    rows = score_catalog(m, _csr(d), range(3), strategy=strategy).cpu().numpy()
    total = _check_rows(d, refs, rows, int(m._last_nan.item()), ("band", precision, D, H, strategy))
    assert total == len(d.band_c)
    print("band", precision, D, H, strategy, "NaN candidates compared:", total)


@pytest.mark.parametrize("D,H", [(32, 32), (64, 64), (192, 192)])
def test_product_overflow_band_forward(D, H):
    """forward() sums the same rounded products: 1.0, 0.0, and NaN for A + B in either order (a
    product fused into the sum would give the first item's saturation instead, 1.0 or 0.0)."""
    d, _ = _band_ref(D, H)
    m = _model("basic", d.params)
    A, B = d.band_h
    t = d.band_c[[0, 40, -1]]
    got1 = m(_t(np.array([[A], [B], [A]])), _t(np.array([t[0], t[1], 5]))).cpu().numpy()
    assert got1[0] == 1.0 and got1[1] == 0.0 and abs(got1[2] - 0.5) < 0.05 and int(m._last_nan.item()) == 0
    hist = np.array([[A, B], [B, A], [A, B], [A, A], [B, B], [A, B]])
    tgt = np.array([t[0], t[1], t[2], t[0], t[1], 5])
    got = m(_t(hist), _t(tgt)).cpu().numpy()
    assert np.isnan(got[:3]).all() and got[3] == 1.0 and got[4] == 0.0 and abs(got[5] - 0.5) < 0.05, got
    assert int(m._last_nan.item()) == 3
    ref, _ = nais_oracle.forward_basic(d.params, hist, tgt)
    assert np.all(ref[:3] == 0.0)                    # the reference is finite there
    assert np.max(np.abs(ref[3:] - got[3:])) <= SCORE_ATOL


@pytest.mark.parametrize("precision,D,H", BAND_SHAPES)
def test_product_overflow_band_topk_routes(precision, D, H):
    d, refs = _band_ref(D, H)
    m = _model("basic", d.params, precision=precision)
    _assert_gate_refuses(m)
    _all_routes(d, refs, m, K, ("band", precision, D, H))
