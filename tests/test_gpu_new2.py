"""New2 on the device (model.New2, new2.score_topk, validation.New2_validation) against the
reference's fixture (tests/golden/new2.npz) and the float64 oracle (tests/_new2_oracle.py).

Tolerances (derived in the oracle's docstring): two fp32 results within 2 E(u, c); top-k lists by
assert_topk_equivalent with tie_eps = score_atol = 2 max_c E(u, c).
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _new2_oracle as n2
from _new1_oracle import visit_rates
from _helpers import assert_topk_equivalent, load_golden, positives_from
from _new2_common import (FWD, TAGS, fwd_inputs, fwd_oracle, golden_csr, golden_params, golden_rate,
                          make_model, random_params)
from poi_recommendation_models_amd import new1, new2, validation

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def z():
    return load_golden("new2.npz")


@pytest.fixture(scope="module")
def bounds(z):
    """E[tag][u, c] of every user's candidates (NaN on history POIs): computed once, read only."""
    rate, out = golden_rate(z), {}
    for tag in TAGS:
        p = golden_params(z, tag)
        E = np.full((int(z["num_users"]), int(z["num_pois"])), np.nan)
        for u in range(E.shape[0]):
            cands, _, e = n2.user_row(p, float(z["beta"]), z["indptr"], z["indices"], rate,
                                      z["region_of"], z["dist"], u)
            E[u, cands] = e
        E.setflags(write=False)
        out[tag] = E
    return out


class _Args:
    topk = 50


def eval_forward(m, indptr, indices, rate, region_of, dist32, u):
    """The evaluation batch of user u through model.forward on the device: the shared history as
    an expanded view, the [n, b] distance block as the dataset slices it. (cands, scores)."""
    lo, hi = int(indptr[u]), int(indptr[u + 1])
    h = np.asarray(indices[lo:hi], dtype=np.int64)
    cands = np.setdiff1d(np.arange(dist32.shape[0], dtype=np.int64), h)
    b = len(cands)
    hist, c = torch.from_numpy(h).to(DEV), torch.from_numpy(cands).to(DEV)
    reg = torch.from_numpy(np.asarray(region_of, dtype=np.int64)).to(DEV)
    block = torch.from_numpy(np.ascontiguousarray(dist32[h][:, cands])).to(DEV)
    with torch.no_grad():
        got = m(hist.unsqueeze(0).expand(b, -1), c, reg[hist].unsqueeze(0).expand(b, -1), reg[c],
                torch.from_numpy(np.asarray(rate[lo:hi])).to(DEV), block, torch.tensor(u))
    return cands, got.cpu().numpy()


# ---- 1. golden forward cases
@pytest.mark.parametrize("tag", TAGS)
def test_golden_forward(z, tag):
    p, beta = golden_params(z, tag), float(z["beta"])
    m = make_model(p, beta, DEV)
    with torch.no_grad():
        for b, n in FWD:
            arrs, tens = fwd_inputs(z, b, n, DEV)
            _, E = fwd_oracle(p, beta, arrs)
            ref = z[f"{tag}/fwd{b}x{n}/prediction"]
            got = m(*tens).cpu().numpy()
            rest = m.restatement(*tens).cpu().numpy()
            print(tag, b, n, "kernel / restatement: max dev / 2E",
                  float((np.abs(got - ref) / (2 * E)).max()), float((np.abs(rest - ref) / (2 * E)).max()))
            assert np.all(np.abs(got - ref) <= 2 * E), (b, n)
            assert np.all(np.abs(rest - ref) <= 2 * E), (b, n)
            assert np.array_equal(m(*[t.unsqueeze(0) for t in tens[:6]], tens[6]).cpu().numpy(), got)


# ---- 2. golden evaluation
@pytest.mark.parametrize("source", ("dist_mat", "coords"))
@pytest.mark.parametrize("tag", TAGS)
def test_score_topk_lists_and_scores(z, bounds, tag, source):
    m = make_model(golden_params(z, tag), float(z["beta"]), DEV)
    U = int(z["num_users"])
    kw = {"dist_mat": z["dist"]} if source == "dist_mat" else {"coords": z["coords"]}
    ids_t, sc_t = new2.score_topk(m, golden_csr(z), z["region_of"], range(U), 50, **kw)
    assert int(m._last_short.item()) == 0
    ids, sc = ids_t.cpu().numpy(), sc_t.cpu().numpy()
    E, worst = bounds[tag], 0.0
    for u in range(U):
        emax = float(np.nanmax(E[u]))
        row = z[f"{tag}/rows"][u]
        assert not np.isnan(row[ids[u]]).any(), "a history POI was recommended"
        worst = max(worst, float((np.abs(sc[u] - row[ids[u]]) / (2 * E[u, ids[u]])).max()))
        assert np.all(np.abs(sc[u] - row[ids[u]]) <= 2 * E[u, ids[u]]), u
        assert_topk_equivalent(z[f"{tag}/topk_ids"][u], z[f"{tag}/topk_scores"][u], ids[u], sc[u],
                               tie_eps=2 * emax, score_atol=2 * emax,
                               lookup={int(c): float(row[c]) for c in np.flatnonzero(~np.isnan(row))})
    print(tag, source, "scorer vs reference: max dev / 2E", worst)


def test_validation_six_tuple(z):
    m = make_model(golden_params(z, "spread"), float(z["beta"]), DEV).train()
    got = validation.New2_validation(m, _Args(), int(z["num_users"]), positives_from(z, "test"),
                                     positives_from(z, "val"), golden_csr(z), z["region_of"],
                                     z["coords"], z["k_list"].tolist())
    assert not m.training
    np.testing.assert_array_equal(np.array(got, dtype=np.float64), z["spread/metrics"])


@pytest.mark.parametrize("tag", TAGS)
def test_golden_rows_through_forward(z, bounds, tag):
    m = make_model(golden_params(z, tag), float(z["beta"]), DEV)
    rate = visit_rates(z["indptr"], z["indices"], z["data"], int(z["num_pois"]))
    worst = 0.0
    for u in range(int(z["num_users"])):
        cands, got = eval_forward(m, z["indptr"], z["indices"], rate, z["region_of"], z["dist"], u)
        dev = np.abs(got - z[f"{tag}/rows"][u, cands])
        worst = max(worst, float((dev / (2 * bounds[tag][u, cands])).max()))
        assert np.all(dev <= 2 * bounds[tag][u, cands]), u
    print(tag, "rows: max dev / 2E", worst)


# ---- 3. the scorer against the forward on shapes chosen for the index arithmetic
def run_of(lo, hi):
    return list(range(lo, hi))


def synthetic(seed, P, d, R, hists, zero_rows=(), balanced=None, scale=0.1):
    """A small job: seeded parameters (embeddings N(0, scale), small enough that few scores
    saturate), coordinates in the Tokyo box, visit counts 1..5."""
    rng = np.random.default_rng(seed)
    U = len(hists)
    p = random_params(rng, P, d, R, U, scale=scale)
    for u in zero_rows:
        p["embed_dist"][u] = 0.0
    region_of = rng.integers(0, R, P).astype(np.int64)
    if balanced is not None:      # user `balanced`: w = (+1/2, -1/2), regions alternate
        region_of = (np.arange(P) % 2).astype(np.int64)
        p["embed_dist"][balanced] = (0.5, -0.5)
    indptr = np.cumsum([0] + [len(h) for h in hists]).astype(np.int64)
    indices = np.array(sum([sorted(h) for h in hists], []), dtype=np.int64)
    data = rng.integers(1, 6, len(indices)).astype(np.float64)
    coords = np.stack([rng.uniform(35.5, 35.8, P), rng.uniform(139.5, 139.9, P)], 1)
    coords[1] = coords[0]                                           # a distance of exactly 0
    dist32 = n2.haversine_km(coords, coords).astype(np.float32)
    X = sp.csr_matrix((data, indices, indptr), shape=(U, P))
    rate = visit_rates(indptr, indices, data, P)
    return dict(p=p, P=P, X=X, indptr=indptr, indices=indices, region_of=region_of, coords=coords,
                dist=dist32, rate=rate, rate32=rate.astype(np.float32).astype(np.float64))


def check_scorer_against_forward(job, users, num_chunks=0, beta=0.5):
    m = make_model(job["p"], beta, DEV)
    tabs = new1.catalog_tables(m, job["region_of"])
    for u in users:
        cands, s, E = n2.user_row(job["p"], beta, job["indptr"], job["indices"], job["rate32"],
                                  job["region_of"], job["dist"], u)
        b, emax = len(cands), float(np.nanmax(E))
        k = min(b, 256)
        s32 = s.astype(np.float32)
        assert np.mean((s32 == 0) | (s32 == 1)) < 0.25, "saturated scores compare nothing"
        fc, fwd = eval_forward(m, job["indptr"], job["indices"], job["rate"], job["region_of"],
                               job["dist"], u)
        assert np.array_equal(fc, cands) and np.all(np.abs(fwd - s) <= E), u
        lut = dict(zip(cands.tolist(), fwd.tolist()))
        Eof = dict(zip(cands.tolist(), E.tolist()))
        oi, osc = n2.topk(cands, s, k)
        for kw in ({"dist_mat": job["dist"]}, {"coords": job["coords"]}):
            ids_t, sc_t = new2.score_topk(m, job["X"], job["region_of"], [u], k, num_chunks=num_chunks,
                                          tables=tabs, **kw)
            assert int(m._last_short.item()) == 0
            ids, sc = ids_t.cpu().numpy()[0], sc_t.cpu().numpy()[0]
            assert set(ids.tolist()) <= set(cands.tolist()), "a history POI was recommended"
            dev = np.array([abs(sc[i] - lut[int(c)]) / (2 * Eof[int(c)]) for i, c in enumerate(ids)])
            print("user", u, "n", job["indptr"][u + 1] - job["indptr"][u], list(kw)[0],
                  "scorer vs forward: max dev / 2E", float(dev.max()))
            assert np.all(dev <= 1.0), (u, list(kw)[0], float(dev.max()))
            assert_topk_equivalent(oi, osc, ids, sc, tie_eps=2 * emax, score_atol=2 * emax,
                                   lookup=dict(zip(cands.tolist(), s.tolist())))


def test_scorer_index_arithmetic_d64():
    """d = 64 (JB = 224): n = 2, 31, 33 and 230 (two history blocks: the parked sums and a block
    boundary), a history holding ids 0, P - 1 and a run of consecutive ids, a zero embed_dist row
    (sigma_u = 0, omega = 0); the run history belongs to the last user id."""
    P = 280
    rng = np.random.default_rng(64)
    hists = [rng.choice(P, n, replace=False).tolist() for n in (2, 31, 33, 230, 20)]
    hists.append([0, P - 1] + run_of(100, 117) + [5, 7, 250])
    job = synthetic(1, P, 64, 7, hists, zero_rows=(4,))
    check_scorer_against_forward(job, range(len(hists)))


def test_scorer_index_arithmetic_d16_one_region():
    P = 200
    rng = np.random.default_rng(16)
    hists = [rng.choice(P, n, replace=False).tolist() for n in (2, 31, 33)]
    hists.append([0, P - 1] + run_of(60, 90))
    check_scorer_against_forward(synthetic(2, P, 16, 1, hists), range(len(hists)))


def test_scorer_index_arithmetic_d130_sigma_zero():
    """d = 130 (the instance without operand registers) and a user whose sigma_u is exactly 0 with
    non-zero weights: w = (1/2, -1/2), regions alternating, a history with as many even as odd ids."""
    P = 210
    rng = np.random.default_rng(130)
    hists = [rng.choice(P, n, replace=False).tolist() for n in (31, 33)]
    hists.append(run_of(10, 20) + run_of(101, 111) + [150, 153])
    job = synthetic(3, P, 130, 2, hists, balanced=2, scale=0.05)
    cands = np.setdiff1d(np.arange(P), hists[2])
    assert job["p"]["embed_dist"][2][job["region_of"][cands]].astype(np.float64).sum() == 0.0
    check_scorer_against_forward(job, range(len(hists)))


def test_scorer_more_history_than_candidates():
    """P = 12, n = 8, b = 4: a row's positions wrap past b more than once (forward and scorer)."""
    job = synthetic(4, 12, 16, 3, [[0, 1, 2, 4, 6, 7, 9, 11], [3, 5]])
    check_scorer_against_forward(job, (0, 1))


def test_scorer_chunk_boundary_on_a_wrapping_row():
    """Three column chunks of 256; the candidate at the first boundary (POI 256) has a row whose
    position index wraps past b."""
    P, n = 600, 33
    rng = np.random.default_rng(7)
    for _ in range(1000):
        h = np.sort(rng.choice(P, n, replace=False))
        if 256 in h:
            continue
        pos, b = 256 - int(np.sum(h < 256)), P - n
        if (pos * n) % b + n > b:
            break
    else:
        raise AssertionError("no such history")
    job = synthetic(5, P, 64, 9, [h.tolist(), rng.choice(P, 40, replace=False).tolist()])
    check_scorer_against_forward(job, (0, 1), num_chunks=4)


# ---- 4. geo edges in one batch
def test_geo_edges_and_nan_pattern(z):
    p, beta = golden_params(z, "spread"), float(z["beta"])
    m = make_model(p, beta, DEV)
    arrs, _ = fwd_inputs(z, 40, 13)
    G, _ = n2.geo_terms(p, arrs[2], arrs[3], arrs[5], arrs[6])
    assert (G > 0).any() and (G < 0).any()
    dist = arrs[5].astype(np.float32).reshape(-1).copy()            # flat [b * n]: row c at c * n
    dist[0 * 13 + 1] = 0.0                                          # geo = 1
    dist[1 * 13: 2 * 13] = 1.0e4                                    # expf underflows: geo = 0
    dist[2 * 13 + 3] = np.nan                                       # a NaN distance: a NaN row
    arrs[5] = dist
    s, E = fwd_oracle(p, beta, arrs)
    tens = [torch.from_numpy(np.asarray(a)).to(DEV) for a in arrs]
    with torch.no_grad():
        got, rest = m(*tens).cpu().numpy(), m.restatement(*tens).cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(rest)) and np.array_equal(np.isnan(got), np.isnan(s))
    assert np.isnan(got[2]) and np.isnan(got).sum() == 1
    ok = ~np.isnan(s)
    assert np.all(np.abs(got[ok] - rest[ok]) <= 2 * E[ok]) and np.all(np.abs(got[ok] - s[ok]) <= E[ok])


# ---- 5. errors
def test_errors(z):
    m = make_model(golden_params(z, "init"), float(z["beta"]), DEV)
    _, tens = fwd_inputs(z, 7, 5, DEV)
    with torch.no_grad():
        for i, bad in ((0, 300), (1, -1), (2, 12), (3, 12)):
            t = [x.clone() for x in tens]
            t[i].view(-1)[0] = bad
            with pytest.raises(IndexError):
                m(*t)
        for bad in (24, -1):
            with pytest.raises(IndexError):
                m(*tens[:6], torch.tensor(bad))
        with pytest.raises(ValueError, match="dist_mat"):
            m(*tens[:5], tens[5][:, :6], tens[6])
    X = golden_csr(z)
    with pytest.raises(ValueError, match="exactly one"):
        new2.score_topk(m, X, z["region_of"], range(3), 5)
    with pytest.raises(ValueError, match="exactly one"):
        new2.score_topk(m, X, z["region_of"], range(3), 5, coords=z["coords"], dist_mat=z["dist"])
    with pytest.raises(IndexError):
        new2.score_topk(m, X, z["region_of"], [24], 5, coords=z["coords"])

    class A:
        topk = 299

    with pytest.raises(RuntimeError, match="selected index k out of range"):
        validation.New2_validation(m, A(), 3, [[1]] * 3, [[2]] * 3, X, z["region_of"], z["coords"], [5])


# ---- 6. grad mode
def test_grad_mode_forward_and_backward(z):
    p, beta = golden_params(z, "spread"), float(z["beta"])
    m = make_model(p, beta, DEV).train()
    arrs, tens = fwd_inputs(z, 40, 13, DEV)
    _, E = fwd_oracle(p, beta, arrs)
    pred = m(*tens)
    assert pred.requires_grad
    with torch.no_grad():
        kern = m(*tens)
    assert np.all(np.abs(pred.detach().cpu().numpy() - kern.cpu().numpy()) <= 2 * E)
    assert np.all(np.abs(pred.detach().cpu().numpy() - z["spread/fwd40x13/prediction"]) <= 2 * E)
    m.loss_function(pred, torch.zeros(40, device=DEV)).backward()
    params = dict(m.named_parameters())
    assert len(params) == 6
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in params.values())
    g, uid = m.embed_dist.grad.cpu(), int(arrs[6])
    other = torch.arange(g.shape[0]) != uid
    assert g[uid].abs().sum() > 0 and not g[other].any()


# ---- 7. determinism
def test_score_topk_is_deterministic(z):
    m = make_model(golden_params(z, "spread"), float(z["beta"]), DEV)
    runs = [new2.score_topk(m, golden_csr(z), z["region_of"], range(int(z["num_users"])), 50,
                            coords=z["coords"], num_chunks=nc) for nc in (0, 0, 2, 2)]
    for a, b in ((0, 1), (2, 3)):
        assert torch.equal(runs[a][0], runs[b][0])
        assert torch.equal(runs[a][1].view(torch.int32), runs[b][1].view(torch.int32))
