"""BPR on the device (model.BPR, bpr.score_topk, validation.BPR_validation, trainer.BPRTrainer)
against the reference's fixture (tests/golden/bpr.npz) and the float64 oracle (tests/_bpr_oracle.py).

Score tolerance (derived, tests/_bpr_oracle.py): E(u, c) = 2 (D + 1) 2^-24 sum_e |U[u,e] I[c,e]|.
Top-k lists: assert_topk_equivalent with tie_eps = 2 max_c E(u, c), score_atol = max_c E(u, c).
Gradients: within GRAD_RTOL x max|g| of their tensor; post-step elements within
lr GRAD_RTOL max|g| + one fp32 ulp; NaN / inf patterns identical.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _bpr_oracle as bo
from _helpers import (GRAD_RTOL, assert_topk_equivalent, load_golden, params_from, positives_from,
                      ulp32)
from poi_recommendation_models_amd import bpr, validation
from poi_recommendation_models_amd.model import BPR
from poi_recommendation_models_amd.trainer import BPRTrainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAGS = ("init", "spread")
LR = 0.01


@pytest.fixture(scope="module")
def z():
    return load_golden("bpr.npz")


def _model(U, I):
    m = BPR(U.shape[0], I.shape[0], U.shape[1])
    m.load_state_dict({"embed_user.weight": torch.from_numpy(np.ascontiguousarray(U, np.float32)),
                       "embed_item.weight": torch.from_numpy(np.ascontiguousarray(I, np.float32))})
    return m.to(DEV)


def _golden_model(z, tag):
    p = params_from(z, tag)
    return _model(p["embed_user.weight"], p["embed_item.weight"]), p["embed_user.weight"], p["embed_item.weight"]


def _golden_csr(z):
    return sp.csr_matrix((np.ones(len(z["indices"])), z["indices"], z["indptr"]),
                         shape=(int(z["num_users"]), int(z["num_pois"])))


def _csr(hists, P):
    indptr = np.concatenate([[0], np.cumsum([len(h) for h in hists])]).astype(np.int64)
    indices = np.concatenate([np.asarray(h, np.int64) for h in hists] + [np.zeros(0, np.int64)])
    return sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(len(hists), P))


def _pair_E(U, I, u, c):
    return 2.0 * (U.shape[1] + 1) * 2.0 ** -24 * np.sum(np.abs(U[u].astype(np.float64) * I[c]), -1)


def _dev(a):
    return torch.from_numpy(np.asarray(a, np.int64)).to(DEV)


def _rescore_bits(m, ids, sc):
    """Every returned (u, id) through model.forward: the same score bits."""
    n, k = ids.shape
    ok = ids >= 0
    u = torch.arange(n, device=DEV).unsqueeze(1).expand(n, k)[ok]
    with torch.no_grad():
        p, _ = m(u, ids[ok], ids[ok])
    assert torch.equal(p.view(torch.int32), sc[ok].view(torch.int32))


def _check_topk(U, I, hists, k, exact_ids=False, **kw):
    """bpr.score_topk of every user against the oracle; returns (ids, scores) as numpy."""
    P = I.shape[0]
    m = _model(U, I)
    ids_t, sc_t = bpr.score_topk(m, _csr(hists, P), range(len(hists)), k, **kw)
    _rescore_bits(m, ids_t, sc_t)
    ids, sc = ids_t.cpu().numpy(), sc_t.cpu().numpy()
    rows, Em = bo.scores(U, I), bo.E(U, I)
    short = 0
    for u, hist in enumerate(hists):
        rid, rsc = bo.topk(rows[u], hist, k)
        c = len(rid)
        short += c < k
        assert np.all(ids[u, c:] == -1) and np.all(np.isnan(sc[u, c:]))
        assert not set(ids[u, :c].tolist()) & set(int(x) for x in hist)
        if exact_ids:
            assert np.array_equal(ids[u, :c], rid), u
            continue
        fin = Em[u][np.isfinite(Em[u])]
        emax = float(fin.max()) if len(fin) else 0.0
        assert_topk_equivalent(rid, rsc, ids[u, :c], sc[u, :c], tie_eps=2 * emax, score_atol=emax,
                               lookup=dict(enumerate(rows[u].tolist())))
    assert int(m._last_short.item()) == short
    return ids, sc


# ------------------------------------------------------------------------------------------ golden
@pytest.mark.parametrize("tag", TAGS)
def test_golden_forward_and_rows(z, tag):
    m, U, I = _golden_model(z, tag)
    assert all(torch.equal(v.cpu(), torch.from_numpy(z[f"{tag}/{k}"])) for k, v in m.state_dict().items())
    with torch.no_grad():
        for n in (1, 7, 33):
            pre = f"{tag}/fwd{n}/"
            u, i, j = z[pre + "user"], z[pre + "item_i"], z[pre + "item_j"]
            pi, pj = m(_dev(u), _dev(i), _dev(j))
            assert np.all(np.abs(pi.cpu().numpy() - z[pre + "prediction_i"]) <= _pair_E(U, I, u, i))
            assert np.all(np.abs(pj.cpu().numpy() - z[pre + "prediction_j"]) <= _pair_E(U, I, u, j))
        nu, P = U.shape[0], I.shape[0]
        uu = torch.arange(nu, device=DEV).repeat_interleave(P)
        cc = torch.arange(P, device=DEV).repeat(nu)
        rows = m(uu, cc, cc)[0].reshape(nu, P).cpu().numpy()
    ref = z[f"{tag}/rows"]
    cand = ~np.isnan(ref)
    assert np.all(np.abs(rows - ref)[cand] <= bo.E(U, I)[cand])


@pytest.mark.parametrize("tag", TAGS)
def test_golden_topk_and_validation(z, tag):
    m, U, I = _golden_model(z, tag)
    X = _golden_csr(z)
    ids, sc = bpr.score_topk(m, X, range(U.shape[0]), 50)
    _rescore_bits(m, ids, sc)
    ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
    assert np.array_equal(ids, z[f"{tag}/topk_ids"])          # position by position, nothing excused
    assert np.all(np.abs(sc - z[f"{tag}/topk_scores"]) <= bo.E(U, I).max(1)[:, None])

    class A:
        topk = 50
    got = validation.BPR_validation(m, A(), U.shape[0], positives_from(z, "test"),
                                    positives_from(z, "val"), X, [int(x) for x in z["k_list"]])
    assert np.array_equal(np.array(got, dtype=np.float64), z[f"{tag}/metrics"])


# ---------------------------------------------------------------------- shapes against the oracle
def _hists(rng, nu, P, k):
    lens = [h for h in (0, 1, 32, 33, P - k, P - 3) if 0 <= h <= P]
    return [np.sort(rng.choice(P, lens[u % len(lens)], replace=False)) for u in range(nu)]


def _random_case(nu, P, D, k, seed=0, **kw):
    rng = np.random.default_rng(seed)
    U = (0.3 * rng.standard_normal((nu, D))).astype(np.float32)
    I = (0.3 * rng.standard_normal((P, D))).astype(np.float32)
    return _check_topk(U, I, _hists(rng, nu, P, k), k, **kw)


@pytest.mark.parametrize("D", [1, 2, 3, 31, 33, 64, 128, 200, 256])
def test_shapes_embed_dim(D):
    _random_case(33, 1000, D, 50, seed=D)


@pytest.mark.parametrize("nu", [1, 31, 33, 70])
@pytest.mark.parametrize("P", [33, 1000, 5003])
def test_shapes_users_pois(nu, P):
    _random_case(nu, P, 31, min(50, P), seed=nu + P)


@pytest.mark.parametrize("k", [1, 50, 256])
def test_shapes_k(k):
    _random_case(33, 5003, 33, k, seed=k)
    _random_case(7, 300, 8, k, seed=k + 1)      # k = 256 of at most 300 candidates: short lists


# ------------------------------------------------------------------------------------ adversarial
def test_best_scores_all_in_history():
    rng = np.random.default_rng(1)
    U = (0.3 * rng.standard_normal((5, 24))).astype(np.float32)
    I = (0.3 * rng.standard_normal((1200, 24))).astype(np.float32)
    rows = bo.scores(U, I)
    hists = [np.sort(np.argsort(-rows[u])[:60]) for u in range(5)]
    ids, _ = _check_topk(U, I, hists, 50)
    for u in range(5):
        assert np.array_equal(ids[u], np.argsort(-rows[u])[60:110])


def test_all_negative_and_zero_user_row():
    rng = np.random.default_rng(2)
    U = np.abs(0.3 * rng.standard_normal((6, 16))).astype(np.float32)
    I = -np.abs(0.3 * rng.standard_normal((900, 16))).astype(np.float32)
    U[3] = 0.0
    hists = [np.sort(rng.choice(900, 20, replace=False)) for _ in range(6)]
    hists[3] = np.array([0, 2, 5, 40])
    ids, sc = _check_topk(U, I, hists, 50)
    assert np.all(sc[[0, 1, 2, 4, 5]] < 0)
    assert np.array_equal(ids[3], np.setdiff1d(np.arange(900), hists[3])[:50])   # the 50 lowest ids
    assert np.all(sc[3] == 0) and not np.any(np.signbit(sc[3]))


def test_exact_ties_straddling_k():
    rng = np.random.default_rng(3)
    U = np.abs(0.3 * rng.standard_normal((4, 12))).astype(np.float32)
    I = (0.05 * rng.standard_normal((2000, 12))).astype(np.float32)
    I[300:340] = np.abs(I[7]) + 1.0        # 40 identical rows, the best scores of every user
    I[900:930] = np.abs(I[8]) + 0.5        # 30 more: the block that straddles rank 50
    hists = [np.array([305, 910]), np.zeros(0, np.int64), np.array([1, 2, 3]), np.arange(300, 320)]
    ids, sc = _check_topk(U, I, hists, 50)
    for u in range(4):
        for s in np.unique(sc[u]):
            run = ids[u][sc[u] == s]
            assert np.all(np.diff(run) > 0)            # exact ties: ascending POI id
        exp = np.concatenate([np.setdiff1d(np.arange(300, 340), hists[u]),
                              np.setdiff1d(np.arange(900, 930), hists[u])])[:50]
        assert np.array_equal(ids[u], exp)


def test_nan_item_row_comes_first():
    rng = np.random.default_rng(4)
    U = (0.3 * rng.standard_normal((3, 10))).astype(np.float32)
    I = (0.3 * rng.standard_normal((700, 10))).astype(np.float32)
    I[77, 3] = np.nan
    hists = [np.array([5, 77, 80]), np.array([9]), np.zeros(0, np.int64)]
    ids, sc = _check_topk(U, I, hists, 50)
    assert 77 not in ids[0] and not np.isnan(sc[0]).any()
    for u in (1, 2):
        assert ids[u, 0] == 77 and np.isnan(sc[u, 0]) and not np.isnan(sc[u, 1:]).any()


def test_infinite_scores():
    rng = np.random.default_rng(5)
    U = (0.3 * rng.standard_normal((4, 6))).astype(np.float32)
    I = (0.3 * rng.standard_normal((33, 6))).astype(np.float32)
    U[:, 0] = [1.0, -1.0, 2.0, -0.5]
    I[5, 0], I[6, 0] = np.inf, -np.inf
    hists = [np.array([0, 1, 2]), np.array([0, 1, 2]), np.array([3]), np.array([5, 9, 11])]
    m = _model(U, I)
    ids, sc = bpr.score_topk(m, _csr(hists, 33), range(4), 30)
    _rescore_bits(m, ids, sc)
    ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
    rows = bo.scores(U, I)
    for u in range(4):
        rid, rsc = bo.topk(rows[u], hists[u], 30)
        assert np.array_equal(ids[u, :len(rid)], rid)
        assert np.array_equal(np.isinf(sc[u, :len(rid)]), np.isinf(rsc))
        assert np.array_equal(sc[u, :len(rid)][np.isinf(rsc)], rsc[np.isinf(rsc)])
    assert sc[0, 0] == np.inf and sc[0, 29] == -np.inf and sc[1, 0] == np.inf and ids[1, 0] == 6


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("k", [50, 256])
def test_monotone_scores_stress_compaction(sign, k):
    P = 5003
    U = np.ones((3, 1), np.float32)
    I = (sign * np.arange(P, dtype=np.float32) / 1024.0).reshape(P, 1)    # exact in fp32
    hists = [np.zeros(0, np.int64), np.arange(P - 40, P), np.arange(0, 40)]
    _check_topk(U, I, hists, k, exact_ids=True)
    _check_topk(U, I, hists, k, exact_ids=True, num_chunks=3)


def test_column_chunk_count_does_not_change_keys():
    rng = np.random.default_rng(6)
    U = (0.3 * rng.standard_normal((37, 20))).astype(np.float32)
    I = (0.3 * rng.standard_normal((5003, 20))).astype(np.float32)
    I[1000:1040] = I[999]                                    # ties across a chunk boundary too
    hists = _hists(rng, 37, 5003, 50)
    m, X = _model(U, I), _csr(hists, 5003)
    base = None
    for nc in (1, 0, 2, 3, 7, 40):
        _, _, keys, cnt = bpr.score_topk(m, X, range(37), 50, num_chunks=nc, return_keys=True)
        keys, cnt = keys.cpu().numpy(), cnt.cpu().numpy()
        keys = np.where(np.arange(50)[None, :] < cnt[:, None], keys, 0)
        if base is None:
            base = (keys, cnt)
        assert np.array_equal(keys, base[0]) and np.array_equal(cnt, base[1]), nc


# --------------------------------------------------------------------------------------- training
def _assert_step(o, U, I, uu, tt, loss, pred, grads, lr, tol_scale=1.0):
    """Device results of one step from tables (U, I) against the oracle's dict `o`."""
    ii, jj = tt
    assert np.all(np.abs(pred["prediction_i"].cpu().numpy() - o["pred_i"]) <= _pair_E(U, I, uu, ii))
    assert np.all(np.abs(pred["prediction_j"].cpu().numpy() - o["pred_j"]) <= _pair_E(U, I, uu, jj))
    gmax = {}
    for k, g in (("embed_user.weight", o["grad_user"]), ("embed_item.weight", o["grad_item"])):
        gmax[k] = np.abs(g).max()
        assert np.all(np.abs(grads[k].cpu().numpy() - g) <= tol_scale * GRAD_RTOL * gmax[k]), k
    return gmax


def _assert_tables(m, new_u, new_i, gmax, lr, steps=1):
    for k, ref in (("embed_user.weight", new_u), ("embed_item.weight", new_i)):
        got = m.state_dict()[k].cpu().numpy()
        assert np.all(np.abs(got - ref) <= steps * (lr * GRAD_RTOL * gmax[k] + ulp32(ref))), k


@pytest.mark.parametrize("wd,name", [(0.0, "wd0"), (1e-3, "wd1e-3")])
@pytest.mark.parametrize("tag", TAGS)
def test_golden_training_step(z, tag, wd, name):
    m, U, I = _golden_model(z, tag)
    pre = f"{tag}/train/"
    uu, ii, jj = z[pre + "user"], z[pre + "item_i"], z[pre + "item_j"]
    tr = BPRTrainer(m, _golden_csr(z), lr=LR, weight_decay=wd)
    pred, grads = {}, {}
    tr.step(_dev(uu), _dev(ii), _dev(jj), pred=pred, grads=grads)
    loss = tr.finish()
    ref_loss = float(z[pre + "loss"])
    # n log terms summed in fp32 twice (ours, the reference's), each term within a few ulps
    assert abs(loss - ref_loss) <= 2 * (len(uu) + 8) * 2.0 ** -24 * abs(ref_loss)
    assert np.all(np.abs(pred["prediction_i"].cpu().numpy() - z[pre + "prediction_i"]) <= _pair_E(U, I, uu, ii))
    assert np.all(np.abs(pred["prediction_j"].cpu().numpy() - z[pre + "prediction_j"]) <= _pair_E(U, I, uu, jj))
    gmax = {}
    for k in ("embed_user.weight", "embed_item.weight"):
        gref = z[pre + "grad/" + k]
        gmax[k] = np.abs(gref).max()
        assert np.all(np.abs(grads[k].cpu().numpy() - gref) <= GRAD_RTOL * gmax[k]), k
    _assert_tables(m, bo.post_step_table(z, tag, name, "embed_user.weight"),
                   bo.post_step_table(z, tag, name, "embed_item.weight"), gmax, LR)
    if wd == 0.0:   # untouched rows: bit-identical
        tu = np.setdiff1d(np.arange(U.shape[0]), uu)
        ti = np.setdiff1d(np.arange(I.shape[0]), np.concatenate([ii, jj]))
        assert np.array_equal(m.embed_user.weight.detach().cpu().numpy()[tu].view(np.int32), U[tu].view(np.int32))
        assert np.array_equal(m.embed_item.weight.detach().cpu().numpy()[ti].view(np.int32), I[ti].view(np.int32))


def test_saturated_patterns(z):
    p = params_from(z, "spread")
    U, I = p["embed_user.weight"].copy(), p["embed_item.weight"].copy()
    pre = "saturated/"
    U[z[pre + "user_rows"]] = z[pre + "user_values"]
    I[z[pre + "item_rows"]] = z[pre + "item_values"]
    m = _model(U, I)
    tr = BPRTrainer(m, _golden_csr(z), lr=LR)
    pred, grads = {}, {}
    tr.step(_dev(z[pre + "user"]), _dev(z[pre + "item_i"]), _dev(z[pre + "item_j"]), pred=pred, grads=grads)
    assert tr.finish() == np.inf == float(z[pre + "loss"])
    sat = np.array([True, False, True])                        # x = -100 - 100: exact products
    assert np.array_equal(pred["prediction_i"].cpu().numpy()[sat], z[pre + "prediction_i"][sat])
    assert np.array_equal(pred["prediction_j"].cpu().numpy()[sat], z[pre + "prediction_j"][sat])
    assert np.all(np.abs(pred["prediction_i"].cpu().numpy() - z[pre + "prediction_i"])
                  <= _pair_E(U, I, z[pre + "user"], z[pre + "item_i"]))
    tu, ti = z[pre + "touched_users"], z[pre + "touched_items"]
    for got, ref in ((grads["embed_user.weight"].cpu().numpy()[tu], z[pre + "grad/embed_user.weight"]),
                     (grads["embed_item.weight"].cpu().numpy()[ti], z[pre + "grad/embed_item.weight"]),
                     (m.embed_user.weight.detach().cpu().numpy()[tu], z[pre + "wd0/embed_user.weight"]),
                     (m.embed_item.weight.detach().cpu().numpy()[ti], z[pre + "wd0/embed_item.weight"])):
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(ref).any()
        assert np.array_equal(np.isinf(got), np.isinf(ref))
        ok = np.isfinite(ref)
        gm = np.abs(ref[ok]).max()
        assert np.all(np.abs(got[ok] - ref[ok]) <= GRAD_RTOL * gm)
    # nothing else moved, nothing else is NaN
    assert not np.isnan(np.delete(m.embed_item.weight.detach().cpu().numpy(), ti, 0)).any()


def _toy(seed=8, nu=9, P=60, D=200):
    rng = np.random.default_rng(seed)
    U = (0.3 * rng.standard_normal((nu, D))).astype(np.float32)
    I = (0.3 * rng.standard_normal((P, D))).astype(np.float32)
    # user 2 three times, item 7 as a positive of one triple and a negative of another, item 9
    # twice as a positive, item 11 twice as a negative; users not grouped
    uu = np.array([2, 5, 2, 0, 2, 5, 8])
    ii = np.array([7, 9, 9, 30, 31, 12, 13])
    jj = np.array([11, 7, 11, 40, 41, 42, 7])
    X = sp.csr_matrix((np.ones(len(uu)), (uu, ii)), shape=(nu, P))
    return U, I, uu, ii, jj, X


@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_repeats_and_three_steps_against_oracle(wd):
    U, I, uu, ii, jj, X = _toy()
    m = _model(U, I)
    tr = BPRTrainer(m, X, lr=0.05, weight_decay=wd)
    cu, ci, total = U.astype(np.float64), I.astype(np.float64), 0.0
    for s in range(3):
        before_u = m.embed_user.weight.detach().cpu().numpy().copy()
        before_i = m.embed_item.weight.detach().cpu().numpy().copy()
        o = bo.step(before_u, before_i, uu, ii, jj, 0.05, wd)       # from the device's own state
        pred, grads = {}, {}
        tr.step(_dev(uu), _dev(ii), _dev(jj), pred=pred, grads=grads)
        gmax = _assert_step(o, before_u, before_i, uu, (ii, jj), None, pred, grads, 0.05)
        _assert_tables(m, o["embed_user"], o["embed_item"], gmax, 0.05)
        total += o["loss"]
        if wd == 0.0:
            tu = np.setdiff1d(np.arange(U.shape[0]), uu)
            ti = np.setdiff1d(np.arange(I.shape[0]), np.concatenate([ii, jj]))
            assert np.array_equal(m.embed_user.weight.detach().cpu().numpy()[tu].view(np.int32), before_u[tu].view(np.int32))
            assert np.array_equal(m.embed_item.weight.detach().cpu().numpy()[ti].view(np.int32), before_i[ti].view(np.int32))
    assert abs(tr.finish() - total) <= 1e-5 * abs(total)


def test_step_is_deterministic(z):
    _, U, I = _golden_model(z, "spread")
    pre = "spread/train/"
    args = [_dev(z[pre + k]) for k in ("user", "item_i", "item_j")]
    outs = []
    for _ in range(2):
        m = _model(U, I)
        tr = BPRTrainer(m, _golden_csr(z), lr=LR, weight_decay=1e-3)
        for _ in range(2):
            tr.step(*args)
        outs.append((m.embed_user.weight.detach().clone(), m.embed_item.weight.detach().clone(),
                     tr.loss_sum.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("tag", TAGS)
def test_autograd_route_matches_fixture(z, tag):
    m, U, I = _golden_model(z, tag)
    pre = f"{tag}/train/"
    m.train()
    opt = torch.optim.SGD(m.parameters(), lr=LR)
    opt.zero_grad()
    pi, pj = m(_dev(z[pre + "user"]), _dev(z[pre + "item_i"]), _dev(z[pre + "item_j"]))
    loss = - (pi - pj).sigmoid().log().sum()                    # run.py:506, unchanged
    loss.backward()
    assert abs(loss.item() - float(z[pre + "loss"])) <= 1e-5 * abs(float(z[pre + "loss"]))
    gmax = {}
    for k, v in m.named_parameters():
        gref = z[pre + "grad/" + k]
        gmax[k] = np.abs(gref).max()
        assert np.all(np.abs(v.grad.cpu().numpy() - gref) <= GRAD_RTOL * gmax[k]), k
    opt.step()
    _assert_tables(m, bo.post_step_table(z, tag, "wd0", "embed_user.weight"),
                   bo.post_step_table(z, tag, "wd0", "embed_item.weight"), gmax, LR)


def test_trainer_batch_invariants(z):
    m, U, I = _golden_model(z, "init")
    X = _golden_csr(z)
    indptr, indices, P = z["indptr"], z["indices"], I.shape[0]
    tr = BPRTrainer(m, X)
    users = [5, 0, 9, 17, 5]                                   # h = 60, 0, 1, ...; a user twice
    u, i, j = (t.cpu().numpy() for t in tr.batch(users, seed=123))
    u2, i2, j2 = (t.cpu().numpy() for t in tr.batch(users, seed=123))
    assert np.array_equal(u, u2) and np.array_equal(i, i2) and np.array_equal(j, j2)
    _, _, j3 = (t.cpu().numpy() for t in tr.batch(users, seed=124))
    assert not np.array_equal(j, j3)
    o = 0
    for uid in users:
        hist = indices[indptr[uid]:indptr[uid + 1]]
        h = len(hist)
        assert np.all(u[o:o + h] == uid) and np.array_equal(i[o:o + h], hist)    # CSR order
        neg = j[o:o + h]
        assert len(set(neg.tolist())) == h and not set(neg.tolist()) & set(hist.tolist())
        assert np.all((neg >= 0) & (neg < P))
        o += h
    assert o == len(u)
    tr.finish()
    # more positives than POIs outside the history: the reference's negative[i] raises
    Xbig = _csr([np.arange(0, 40), np.array([1, 2])], 70)
    big = BPRTrainer(_model(U[:2], I[:70]), Xbig)
    with pytest.raises(ValueError):
        big.batch([1, 0])
    a, b, c = big.batch([1])
    assert a.numel() == 2
    # an epoch runs, bumps the parameter versions and returns a finite loss
    v0 = m.embed_user.weight._version
    assert np.isfinite(tr.epoch(batch_size=16))
    assert m.embed_user.weight._version > v0
