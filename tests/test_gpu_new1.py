"""New1 on the device (model.New1, new1.score_topk, validation.New1_validation) against the
reference's fixture (tests/golden/new1.npz) and the float64 oracle (tests/_new1_oracle.py).

Tolerances (derived in the oracle's docstring): two fp32 results -- ours and the reference's --
within 2 E(u, c); top-k lists by assert_topk_equivalent with tie_eps = score_atol = 2 max_c E(u, c).
"""
import numpy as np
import pytest
import torch

import _new1_oracle as no
from _helpers import assert_topk_equivalent, load_golden, positives_from
from _new1_common import FWD, TAGS, fwd_inputs, golden_csr, golden_params, golden_rate, make_model
from poi_recommendation_models_amd import new1, validation

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def z():
    return load_golden("new1.npz")


@pytest.fixture(scope="module")
def bounds(z):
    """E[tag][u, c] of every user's candidates (NaN on history POIs): computed once, read only."""
    rate, out = golden_rate(z), {}
    for tag in TAGS:
        p = golden_params(z, tag)
        E = np.full((int(z["num_users"]), int(z["num_pois"])), np.nan)
        for u in range(E.shape[0]):
            cands, _, e = no.user_row(p, float(z["beta"]), z["indptr"], z["indices"], rate, z["region_of"], u)
            E[u, cands] = e
        E.setflags(write=False)
        out[tag] = E
    return out


class _Args:
    topk = 50


@pytest.mark.parametrize("tag", TAGS)
def test_golden_forward(z, tag):
    p, beta = golden_params(z, tag), float(z["beta"])
    m = make_model(p, beta, DEV)
    with torch.no_grad():
        for b, n in FWD:
            (hist, tgt, hreg, treg, vr), tens = fwd_inputs(z, b, n, DEV)
            _, E = no.forward_rows(p, beta, hist, tgt, hreg, treg, vr.astype(np.float32))
            got = m(*tens).cpu().numpy()
            dev = np.abs(got - z[f"{tag}/fwd{b}x{n}/prediction"])
            print(tag, b, n, "max dev / 2E", float((dev / (2 * E)).max()))
            assert np.all(dev <= 2 * E), (b, n)
            assert np.array_equal(m(*[t.unsqueeze(0) for t in tens]).cpu().numpy(), got)


@pytest.mark.parametrize("tag", TAGS)
def test_golden_rows_through_forward(z, bounds, tag):
    """Every user's candidate row as the reference's validation calls the model: one history
    shared by all rows (an expanded view, read in place)."""
    m = make_model(golden_params(z, tag), float(z["beta"]), DEV)
    rate = torch.from_numpy(no.visit_rates(z["indptr"], z["indices"], z["data"], int(z["num_pois"]))).to(DEV)
    reg = torch.from_numpy(z["region_of"]).to(DEV)
    worst = 0.0
    with torch.no_grad():
        for u in range(int(z["num_users"])):
            lo, hi = int(z["indptr"][u]), int(z["indptr"][u + 1])
            hist = torch.from_numpy(z["indices"][lo:hi]).to(DEV)
            cands = np.setdiff1d(np.arange(int(z["num_pois"])), z["indices"][lo:hi])
            c = torch.from_numpy(cands).to(DEV)
            got = m(hist.unsqueeze(0).expand(len(cands), -1), c, reg[hist].unsqueeze(0).expand(len(cands), -1),
                    reg[c], rate[lo:hi]).cpu().numpy()
            dev = np.abs(got - z[f"{tag}/rows"][u, cands])
            worst = max(worst, float((dev / (2 * bounds[tag][u, cands])).max()))
            assert np.all(dev <= 2 * bounds[tag][u, cands]), u
    print(tag, "rows: max dev / 2E", worst)


def test_overflow_nan_pattern(z):
    p, pre = golden_params(z, "overflow"), "overflow/"
    arrs = [z[pre + k] for k in ("history", "target", "history_region", "target_region", "visit_rate")]
    ref = z[pre + "prediction"]
    m = make_model(p, float(z["beta"]), DEV)
    with torch.no_grad():
        got = m(*[torch.from_numpy(a).to(DEV) for a in arrs]).cpu().numpy()
    _, E = no.forward_rows(p, float(z["beta"]), *arrs[:4], arrs[4].astype(np.float32))
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(ref[:2]).all()
    assert abs(got[2] - ref[2]) <= 2 * E[2]


def test_out_of_range_ids_raise(z):
    m = make_model(golden_params(z, "init"), float(z["beta"]), DEV)
    _, tens = fwd_inputs(z, 7, 5, DEV)
    with torch.no_grad():
        for i, bad in ((0, 700), (1, -1), (2, 16), (3, 16)):
            t = [x.clone() for x in tens]
            t[i].view(-1)[0] = bad
            with pytest.raises(IndexError):
                m(*t)


@pytest.mark.parametrize("tag", TAGS)
def test_score_topk_lists_and_rescore(z, bounds, tag):
    p, beta = golden_params(z, tag), float(z["beta"])
    m = make_model(p, beta, DEV)
    U, P = int(z["num_users"]), int(z["num_pois"])
    ids_t, sc_t = new1.score_topk(m, golden_csr(z), z["region_of"], range(U), 50)
    assert int(m._last_short.item()) == 0
    ids, sc = ids_t.cpu().numpy(), sc_t.cpu().numpy()
    E = bounds[tag]
    for u in range(U):
        emax = float(np.nanmax(E[u]))
        row = z[f"{tag}/rows"][u]
        assert not np.isnan(row[ids[u]]).any(), "a history POI was recommended"
        assert np.all(np.abs(sc[u] - row[ids[u]]) <= 2 * E[u, ids[u]]), u
        assert_topk_equivalent(z[f"{tag}/topk_ids"][u], z[f"{tag}/topk_scores"][u], ids[u], sc[u],
                               tie_eps=2 * emax, score_atol=2 * emax,
                               lookup={int(c): float(row[c]) for c in np.flatnonzero(~np.isnan(row))})
    # every returned (u, id) through model.forward: the two kernels within 2E of each other
    rate = torch.from_numpy(no.visit_rates(z["indptr"], z["indices"], z["data"], P)).to(DEV)
    reg = torch.from_numpy(z["region_of"]).to(DEV)
    worst = 0.0
    with torch.no_grad():
        for u in range(U):
            lo, hi = int(z["indptr"][u]), int(z["indptr"][u + 1])
            hist = torch.from_numpy(z["indices"][lo:hi]).to(DEV)
            f = m(hist.unsqueeze(0).expand(50, -1), ids_t[u], reg[hist].unsqueeze(0).expand(50, -1),
                  reg[ids_t[u]], rate[lo:hi]).cpu().numpy()
            worst = max(worst, float((np.abs(f - sc[u]) / (2 * E[u, ids[u]])).max()))
            assert np.all(np.abs(f - sc[u]) <= 2 * E[u, ids[u]]), u
    print(tag, "scorer vs forward: max dev / 2E", worst)


@pytest.mark.parametrize("tag", ("spread", "sharp"))
def test_validation_six_tuple(z, tag):
    m = make_model(golden_params(z, tag), float(z["beta"]), DEV).train()
    got = validation.New1_validation(m, _Args(), int(z["num_users"]), positives_from(z, "test"),
                                     positives_from(z, "val"), golden_csr(z), z["region_of"],
                                     z["k_list"].tolist())
    assert not m.training
    np.testing.assert_array_equal(np.array(got, dtype=np.float64), z[f"{tag}/metrics"])


def test_validation_raises_when_short(z):
    m = make_model(golden_params(z, "init"), float(z["beta"]), DEV)

    class A:
        topk = 699

    with pytest.raises(RuntimeError, match="selected index k out of range"):
        validation.New1_validation(m, A(), 3, [[1]] * 3, [[2]] * 3, golden_csr(z), z["region_of"], [5])


def test_grad_mode_forward_and_backward(z):
    p, beta = golden_params(z, "spread"), float(z["beta"])
    m = make_model(p, beta, DEV).train()
    (hist, tgt, hreg, treg, vr), tens = fwd_inputs(z, 40, 13, DEV)
    _, E = no.forward_rows(p, beta, hist, tgt, hreg, treg, vr.astype(np.float32))
    pred = m(*tens)
    assert pred.requires_grad
    with torch.no_grad():
        kern = m(*tens)
    assert np.all(np.abs(pred.detach().cpu().numpy() - kern.cpu().numpy()) <= 2 * E)
    assert np.all(np.abs(pred.detach().cpu().numpy() - z["spread/fwd40x13/prediction"]) <= 2 * E)
    m.loss_function(pred, torch.zeros(40, device=DEV)).backward()
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in m.parameters())
