"""tests/_bpr_oracle.py (float64 numpy BPR) pinned to the reference's own results in
tests/golden/bpr.npz (tests/golden/make_golden_bpr.py). CPU only."""
import numpy as np
import pytest

import _bpr_oracle as bo
from _helpers import GRAD_RTOL, load_golden, params_from, ulp32

TAGS = ("init", "spread")
LR = 0.01


@pytest.fixture(scope="module")
def z():
    return load_golden("bpr.npz")


def _tables(z, tag):
    p = params_from(z, tag)
    return p["embed_user.weight"], p["embed_item.weight"]


def _pair_E(U, I, u, c):
    return 2.0 * (U.shape[1] + 1) * 2.0 ** -24 * np.sum(np.abs(U[u].astype(np.float64) * I[c]), -1)


@pytest.mark.parametrize("tag", TAGS)
def test_rows_and_forwards_within_E(z, tag):
    U, I = _tables(z, tag)
    rows, ref = z[f"{tag}/rows"], bo.scores(U, I)
    cand = ~np.isnan(rows)
    indptr, indices = z["indptr"], z["indices"]
    for u in range(len(indptr) - 1):   # exactly the history is missing from a row
        assert np.array_equal(np.flatnonzero(~cand[u]), indices[indptr[u]:indptr[u + 1]])
    assert np.all(np.abs(rows - ref)[cand] <= bo.E(U, I)[cand])
    for n in (1, 7, 33):
        pre = f"{tag}/fwd{n}/"
        u, i, j = z[pre + "user"], z[pre + "item_i"], z[pre + "item_j"]
        assert np.all(np.abs(z[pre + "prediction_i"] - ref[u, i]) <= _pair_E(U, I, u, i))
        assert np.all(np.abs(z[pre + "prediction_j"] - ref[u, j]) <= _pair_E(U, I, u, j))


@pytest.mark.parametrize("tag", TAGS)
def test_topk_lists_and_separation(z, tag):
    U, I = _tables(z, tag)
    ref, tol = bo.scores(U, I), bo.E(U, I).max(1)
    indptr, indices = z["indptr"], z["indices"]
    for u in range(len(indptr) - 1):
        hist = indices[indptr[u]:indptr[u + 1]]
        ids, sc = bo.topk(ref[u], hist, 51)
        assert np.array_equal(ids[:50], z[f"{tag}/topk_ids"][u])
        assert np.all(np.abs(sc[:50] - z[f"{tag}/topk_scores"][u]) <= tol[u])
        # the capture script's separation condition, on the reference's scores
        r = np.sort(np.where(np.isnan(z[f"{tag}/rows"][u]), -np.inf, z[f"{tag}/rows"][u]).astype(np.float64))[::-1]
        assert np.all(r[:50] - r[1:51] > 2 * tol[u])


@pytest.mark.parametrize("wd,name", [(0.0, "wd0"), (1e-3, "wd1e-3")])
@pytest.mark.parametrize("tag", TAGS)
def test_training_step(z, tag, wd, name):
    U, I = _tables(z, tag)
    pre = f"{tag}/train/"
    user, item_i, item_j = z[pre + "user"], z[pre + "item_i"], z[pre + "item_j"]
    o = bo.step(U, I, user, item_i, item_j, LR, wd)
    assert np.all(np.abs(o["pred_i"] - z[pre + "prediction_i"]) <= _pair_E(U, I, user, item_i))
    assert np.all(np.abs(o["pred_j"] - z[pre + "prediction_j"]) <= _pair_E(U, I, user, item_j))
    assert abs(o["loss"] - float(z[pre + "loss"])) <= 1e-5 * abs(o["loss"])
    for k, g, new in (("embed_user.weight", o["grad_user"], o["embed_user"]),
                      ("embed_item.weight", o["grad_item"], o["embed_item"])):
        gref = z[pre + "grad/" + k].astype(np.float64)
        gmax = np.abs(gref).max()
        assert np.all(np.abs(g - gref) <= GRAD_RTOL * gmax)
        pref = bo.post_step_table(z, tag, name, k)
        assert np.all(np.abs(new - pref) <= LR * GRAD_RTOL * gmax + ulp32(pref))


def test_saturated_patterns(z):
    U, I = (a.copy() for a in _tables(z, "spread"))
    pre = "saturated/"
    U[z[pre + "user_rows"]] = z[pre + "user_values"]
    I[z[pre + "item_rows"]] = z[pre + "item_values"]
    o = bo.step(U, I, z[pre + "user"], z[pre + "item_i"], z[pre + "item_j"], LR)
    assert np.isinf(o["loss"]) and np.isinf(float(z[pre + "loss"]))
    tu, ti = z[pre + "touched_users"], z[pre + "touched_items"]
    for got, ref in ((o["grad_user"][tu], z[pre + "grad/embed_user.weight"]),
                     (o["grad_item"][ti], z[pre + "grad/embed_item.weight"]),
                     (o["embed_user"][tu], z[pre + "wd0/embed_user.weight"]),
                     (o["embed_item"][ti], z[pre + "wd0/embed_item.weight"])):
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(ref).any()
        assert np.array_equal(np.isinf(got), np.isinf(ref))
        ok = np.isfinite(ref)
        assert np.allclose(got[ok], ref[ok], rtol=1e-5, atol=1e-7)
