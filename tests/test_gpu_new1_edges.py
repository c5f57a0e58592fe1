"""new1.score_topk and the New1 forward kernel at the edges of their shapes, against the float64
oracle on seeded random parameters (tests/_new1_oracle.py): one fp32 result within E(u, c) of the
oracle, lists by assert_topk_equivalent with tie_eps = 2 max_c E, score_atol = max_c E.

The scorer keeps a candidate's q and t rows in registers up to d = 128 (three compiled widths:
d <= 32, <= 64, <= 128) and reads them in the loop above that; a history longer than the LDS
block (256 rows at d = 66, 128 at d = 130) is walked block by block."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _new1_oracle as no
from _helpers import assert_topk_equivalent
from _new1_common import make_model, random_params
from poi_recommendation_models_amd import new1

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BETA = 0.5


def _case(seed, P, d, R, lens, first_last=False):
    """Seeded parameters, histories of the given lengths with visit counts 1..5, regions."""
    rng = np.random.default_rng(seed)
    params = random_params(rng, P, d, R)
    hists = [np.sort(rng.choice(P, int(n), replace=False)) for n in lens]
    if first_last:   # history ids at 0 and P - 1
        for h in hists:
            if len(h) >= 2:
                h[0], h[-1] = 0, P - 1
    indptr = np.concatenate([[0], np.cumsum([len(h) for h in hists])]).astype(np.int64)
    indices = np.concatenate([*hists, np.zeros(0, np.int64)]).astype(np.int64)
    data = rng.integers(1, 6, len(indices)).astype(np.float64)
    X = sp.csr_matrix((data, indices, indptr), shape=(len(hists), P))
    return params, X, rng.integers(0, R, P).astype(np.int64)


def _check(params, X, region_of, users, k, **kw):
    """score_topk of `users` against the oracle; returns (ids, scores) as numpy."""
    P = X.shape[1]
    m = make_model(params, BETA, DEV)
    ids_t, sc_t = new1.score_topk(m, X, region_of, users, k, **kw)
    ids, sc = ids_t.cpu().numpy(), sc_t.cpu().numpy()
    rate = no.visit_rates(X.indptr, X.indices, X.data, P).astype(np.float32).astype(np.float64)
    short = 0
    for i, u in enumerate(users):
        cands, s, E = no.user_row(params, BETA, X.indptr, X.indices, rate, region_of, u)
        rid, rsc = no.topk(cands, s, k)
        c = len(rid)
        short += c < k
        assert np.all(ids[i, c:] == -1) and np.all(np.isnan(sc[i, c:])), (u, c)
        assert set(ids[i, :c].tolist()) <= set(cands.tolist()), "a history POI was recommended"
        emax = float(E.max()) if len(E) else 0.0
        full_s, full_E = np.full(P, np.nan), np.full(P, np.nan)
        full_s[cands], full_E[cands] = s, E
        assert np.all(np.abs(sc[i, :c] - full_s[ids[i, :c]]) <= full_E[ids[i, :c]]), u
        assert_topk_equivalent(rid, rsc, ids[i, :c], sc[i, :c], tie_eps=2 * emax, score_atol=emax,
                               lookup=dict(zip(cands.tolist(), s.tolist())))
    assert int(m._last_short.item()) == short
    return ids, sc


LENS = (0, 1, 2, 31, 32, 33, 65)


@pytest.mark.parametrize("d", (2, 6, 16, 66, 130))
def test_widths_and_history_lengths(d):
    params, X, reg = _case(d, 129, d, 5, LENS, first_last=True)
    _check(params, X, reg, range(len(LENS)), 50)


@pytest.mark.parametrize("d,n", ((66, 300), (130, 150), (16, 1100)))
def test_history_longer_than_the_lds_block(d, n):
    params, X, reg = _case(100 + d, 2049, d, 7, (n, 3, n + 31))
    _check(params, X, reg, range(3), 50)


@pytest.mark.parametrize("P", (127, 128, 129, 2049))
@pytest.mark.parametrize("k", (1, 50, 256))
def test_catalog_sizes_and_k(P, k):
    params, X, reg = _case(P + k, P, 16, 4, (0, 2, 33, 65))
    _check(params, X, reg, range(4), k)


@pytest.mark.parametrize("k", (1, 50, 256))
def test_exactly_k_candidates(k):
    n = 33
    params, X, reg = _case(k, k + n, 16, 4, (n, n - 1, n + 1))
    _check(params, X, reg, range(X.shape[0]), k)


def test_chunks_give_the_same_keys():
    params, X, reg = _case(11, 2049, 16, 6, (0, 5, 40, 65, 200))
    a_ids, a_sc = _check(params, X, reg, range(5), 50, num_chunks=1)
    b_ids, b_sc = _check(params, X, reg, range(5), 50, num_chunks=3)
    assert np.array_equal(a_ids, b_ids) and np.array_equal(a_sc.view(np.int32), b_sc.view(np.int32))


def test_history_is_nearly_the_whole_catalog():
    P, k = 300, 50
    params, X, reg = _case(5, P, 16, 4, (P - 7, P - k + 1, P - k, P, 10))
    ids, _ = _check(params, X, reg, range(5), k)
    assert (ids[0] >= 0).sum() == 7 and (ids[3] >= 0).sum() == 0 and (ids[2] >= 0).sum() == k


def test_saturated_user_returns_the_lowest_ids():
    P, d, k = 600, 16, 50
    rng = np.random.default_rng(8)
    params = random_params(rng, P, d, 3)
    params["embed_target.weight"][:] = 2.0       # pred >= r * 16 * 4: every sigmoid is 1.0
    params["embed_region.weight"][:] = 2.0
    params["attn_V.weight"][:] = 0.0
    params["attn_Q.weight"][:] = 0.0             # a = 0: every e_j is 1
    hist = np.array([0, 3, 4, 77, P - 1])
    X = sp.csr_matrix((np.ones(5), hist, np.array([0, 5])), shape=(1, P))
    m = make_model(params, BETA, DEV)
    for nc in (1, 3):
        ids, sc = new1.score_topk(m, X, np.zeros(P, np.int64), [0], k, num_chunks=nc)
        assert np.all(sc.cpu().numpy() == 1.0)
        assert ids.cpu().numpy()[0].tolist() == np.setdiff1d(np.arange(P), hist)[:k].tolist()


def test_repeated_users():
    params, X, reg = _case(21, 700, 16, 4, (5, 40, 0))
    ids, sc = _check(params, X, reg, [1, 1, 0, 2, 1, 0], 50)
    assert np.array_equal(ids[0], ids[1]) and np.array_equal(ids[0], ids[4]) and np.array_equal(ids[2], ids[5])
    assert np.array_equal(sc[0].view(np.int32), sc[4].view(np.int32))


@pytest.mark.parametrize("d,n", ((2, 1), (6, 3), (66, 65), (130, 70)))
def test_forward_kernel_against_the_oracle(d, n):
    """The batch forward with per-row histories, targets inside some histories, n = 1 and an
    empty history; an id outside its table raises IndexError."""
    P, R, b = 129, 5, 9
    rng = np.random.default_rng(1000 + d)
    params = random_params(rng, P, d, R)
    m = make_model(params, BETA, DEV)
    hist = np.stack([rng.choice(P, n, replace=False) for _ in range(b)]).astype(np.int64)
    hist[0, 0], hist[1, -1] = 0, P - 1
    tgt = rng.integers(0, P, b).astype(np.int64)
    tgt[3] = hist[3, n // 2]
    hreg, treg = rng.integers(0, R, (b, n)).astype(np.int64), rng.integers(0, R, b).astype(np.int64)
    vr = rng.uniform(0.01, 1.0, n)
    s, E = no.forward_rows(params, BETA, hist, tgt, hreg, treg, vr.astype(np.float32))
    tens = [torch.from_numpy(a).to(DEV) for a in (hist, tgt, hreg, treg, vr)]
    with torch.no_grad():
        got = m(*tens).cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(s))
        ok = ~np.isnan(s)
        assert np.all(np.abs(got[ok] - s[ok]) <= E[ok])
        empty = torch.zeros(b, 0, dtype=torch.int64, device=DEV)
        assert m(empty, tens[1], empty, tens[3], torch.zeros(0, device=DEV)).tolist() == [0.5] * b
        tens[0][2, 0] = P
        with pytest.raises(IndexError):
            m(*tens)
