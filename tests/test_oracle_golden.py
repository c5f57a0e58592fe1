"""Pin the CPU oracle against golden vectors captured from the reference (tests/golden/).

CPU-only. These tests are what make the oracle trustworthy as the GPU parity checker.
"""
import math

import numpy as np
import pytest

from _helpers import (assert_topk_equivalent, family_wide_params, load_golden, params_from,
                      positives_from)
from oracle import metrics_oracle, nais_oracle, powerlaw_oracle

# fp32 CPU restatement vs the reference's torch CPU kernels: different GEMM summation orders
# differ by a few ulps; 1e-6 on sigmoid scores is ~16 ulp at 0.5.
ORACLE_ATOL = 1e-6
ORACLE_TIE_ULPS = 4


@pytest.mark.parametrize("tag", ["init", "trained"])
@pytest.mark.parametrize("n", [1, 5, 20])
def test_forward_basic(tag, n):
    z = load_golden("forward_basic.npz")
    p = params_from(z, tag)
    hist, tgt, ref = z[f"{tag}/n{n}/hist"], z[f"{tag}/n{n}/target"], z[f"{tag}/n{n}/pred"]
    got, nan_count = nais_oracle.forward_basic(p, hist, tgt)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert nan_count == int(np.isnan(ref).sum())
    if n == 1:
        assert nan_count == 8          # rows 0..7: single-item history == target -> 0/0
    ok = ~np.isnan(ref)
    np.testing.assert_allclose(got[ok], ref[ok], rtol=0, atol=ORACLE_ATOL)


@pytest.mark.parametrize("variant", ["region", "region_distance"])
@pytest.mark.parametrize("tag", ["init", "trained"])
@pytest.mark.parametrize("n", [1, 7])
def test_forward_region(variant, tag, n):
    z = load_golden(f"forward_{variant}.npz")
    p = params_from(z, tag)
    region_of = z[f"{tag}/region_of"]
    hist, tgt, ref = z[f"{tag}/n{n}/hist"], z[f"{tag}/n{n}/target"], z[f"{tag}/n{n}/pred"]
    if variant == "region":
        logit = nais_oracle.attention_region(p, hist, tgt, region_of[hist], region_of[tgt])
    else:
        ll = nais_oracle.latlon_pairs(z["coords"], np.broadcast_to(tgt[:, None], hist.shape), hist)
        logit = nais_oracle.attention_region_distance(p, hist, tgt, region_of[hist],
                                                      region_of[tgt], ll.astype(np.float32))
    got = nais_oracle._sigmoid(logit)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    np.testing.assert_allclose(got[ok], ref[ok], rtol=0, atol=ORACLE_ATOL)


@pytest.mark.parametrize("box", ["city", "tight"])
@pytest.mark.parametrize("tag", ["init", "trained"])
@pytest.mark.parametrize("n", [1, 7])
def test_forward_distance(box, tag, n):
    """NAIS_distance_Embedding (model.py:306-408, x1000 distance scale)."""
    z = load_golden("forward_distance.npz")
    p = params_from(z, f"{box}/{tag}")
    pre = f"{box}/{tag}/n{n}/"
    hist, tgt, ref = z[pre + "hist"], z[pre + "target"], z[pre + "pred"]
    ll = nais_oracle.latlon_pairs(z[f"{box}/coords"], np.broadcast_to(tgt[:, None], hist.shape), hist)
    got = nais_oracle._sigmoid(nais_oracle.attention_distance(p, hist, tgt, ll.astype(np.float32)))
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    np.testing.assert_allclose(got[ok], ref[ok], rtol=0, atol=ORACLE_ATOL)


def _catalog(variant, z, p, u):
    P = int(z["num_pois"])
    hist = z["indices"][z["indptr"][u]:z["indptr"][u + 1]]
    if variant == "basic":
        return nais_oracle.catalog_scores_basic(p, hist, P)
    if variant == "region":
        return nais_oracle.catalog_scores_region(p, hist, P, z["region_of"])
    if variant == "distance":
        return nais_oracle.catalog_scores_distance(p, hist, P, z["coords"])
    return nais_oracle.catalog_scores_region_distance(p, hist, P, z["region_of"], z["coords"])


@pytest.mark.parametrize("variant", ["basic", "region", "region_distance", "distance"])
@pytest.mark.parametrize("tag", ["init", "trained"])
def test_catalog_topk(variant, tag):
    z = load_golden(f"catalog_{variant}.npz")
    p = params_from(z, tag)
    U = int(z["num_users"])
    recs = []
    for u in range(U):
        cand, sc = _catalog(variant, z, p, u)
        key = f"{tag}/full_scores_u{u}"
        if key in z.files:
            np.testing.assert_allclose(sc, z[key], rtol=0, atol=ORACLE_ATOL)
        ids, top = nais_oracle.topk_ids(cand, sc, 50)
        lookup = dict(zip(cand.tolist(), sc.tolist()))
        assert_topk_equivalent(z[f"{tag}/topk_ids"][u], z[f"{tag}/topk_scores"][u], ids, top,
                               tie_ulps=ORACLE_TIE_ULPS, lookup=lookup)
        recs.append(ids.tolist())
    # metrics restatement reproduces the reference's 6-tuple on the reference's own lists
    ref_lists = [list(map(int, r)) for r in z[f"{tag}/topk_ids"]]
    k_list = [5, 10, 15, 20, 25, 30]
    val = metrics_oracle.evaluate(positives_from(z, "val"), ref_lists, k_list)
    test = metrics_oracle.evaluate(positives_from(z, "test"), ref_lists, k_list)
    np.testing.assert_array_equal(np.array(val + test), z[f"{tag}/metrics"])


def test_powerlaw_dist_prd_predict():
    z = load_golden("powerlaw.npz")
    d = [powerlaw_oracle.dist(tuple(a), tuple(b)) for a, b in zip(z["dist_a"], z["dist_b"])]
    np.testing.assert_array_equal(np.array(d), z["dist"])
    assert np.all(z["dist"][:80] == 0.0)
    a, b = z["pr_d_ab"]
    np.testing.assert_array_equal(np.array([powerlaw_oracle.pr_d(a, b, x) for x in z["pr_d_in"]]),
                                  z["pr_d"])
    ip, ix, co = z["pl_indptr"], z["pl_indices"], z["pl_coords"]
    fa, fb = powerlaw_oracle.fit(ip, ix, co, *z["fit_w_init"])
    assert (fa, fb) == tuple(z["fit_ab"])
    pred = np.array([[powerlaw_oracle.predict(fa, fb, co, ix[ip[u]:ip[u + 1]], int(c))
                      for c in z["predict_cands"]] for u in range(len(ip) - 1)])
    np.testing.assert_array_equal(pred, z["predict"])
    assert np.all(z["predict"][-1] == 0.0) or np.any(z["predict"][-1] < 1e-300)
    norm = np.array([powerlaw_oracle.normalize(list(r)) for r in z["normalize_in"]])
    np.testing.assert_array_equal(norm, z["normalize"])
    assert powerlaw_oracle.normalize([0.0, 0.0, 0.0]) == list(z["normalize_zero"])
    assert not any(math.isnan(x) for x in d)


def test_train_oracle_golden():
    """Training-step restatement (oracle/train_oracle.py) against the reference's own autograd
    gradients (run.py:101-105 on a get_NAIS_batch batch, dropout off)."""
    from oracle import train_oracle
    z = load_golden("train_step.npz")
    p = {k[2:]: z[k] for k in z.files if k.startswith("p/")}
    r = train_oracle.train_step_basic(p, z["hist"], z["data"], z["labels"])
    assert np.max(np.abs(r["pred"] - z["pred"])) <= 1e-6
    assert abs(r["loss"] - float(z["loss"])) <= 1e-6
    for k, g in r["grads"].items():
        ref = z["grad/" + k]
        assert np.max(np.abs(g.reshape(ref.shape) - ref)) <= 1e-6 * np.abs(ref).max(), k


def test_train_oracle_adagrad_matches_torch():
    import torch
    from oracle import train_oracle
    rng = np.random.default_rng(0)
    p0 = rng.normal(size=(50, 8)).astype(np.float32)
    q = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adagrad([q], lr=0.05, lr_decay=0.1, weight_decay=0.01, foreach=False)
    p, st = p0.copy(), np.zeros_like(p0)
    for step in range(1, 4):
        g = rng.normal(size=p0.shape).astype(np.float32)
        q.grad = torch.from_numpy(g.copy())
        opt.step()
        p, st = train_oracle.adagrad(p, st, g, 0.05, step, lr_decay=0.1, weight_decay=0.01)
    np.testing.assert_allclose(p, q.detach().numpy(), rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("tag", ["init", "trained"])
@pytest.mark.parametrize("n", [1, 7])
def test_forward_new4(tag, n):
    """New4 (model.py:1169-1306) run by the reference with .cuda() as the identity."""
    z = load_golden("new4_forward.npz")
    p = params_from(z, tag)
    hist, tgt, ref = z[f"{tag}/n{n}/hist"], z[f"{tag}/n{n}/target"], z[f"{tag}/n{n}/pred"]
    got = nais_oracle.forward_new4(p, z["near"], p["attn_layer1.weight"].shape[1], hist, tgt)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    np.testing.assert_allclose(got[ok], ref[ok], rtol=0, atol=ORACLE_ATOL)


@pytest.mark.parametrize("tag", ["init", "trained"])
def test_catalog_new4(tag):
    z = load_golden("new4_catalog.npz")
    p = params_from(z, tag)
    P, U = int(z["num_pois"]), int(z["num_users"])
    for u in range(U):
        hist = z["indices"][z["indptr"][u]:z["indptr"][u + 1]]
        cand, sc = nais_oracle.catalog_scores_new4(p, z["near"], 32, hist, P)
        key = f"{tag}/full_scores_u{u}"
        if key in z.files:
            np.testing.assert_allclose(sc, z[key], rtol=0, atol=ORACLE_ATOL)
        ids, top = nais_oracle.topk_ids(cand, sc, 50)
        assert_topk_equivalent(z[f"{tag}/topk_ids"][u], z[f"{tag}/topk_scores"][u], ids, top,
                               tie_ulps=ORACLE_TIE_ULPS, lookup=dict(zip(cand.tolist(), sc.tolist())))


FAMILY = ("New4_padding", "all_in_out", "nearPOI_embedding", "no_POI_emb",
          "transform_ingoing_outgoing", "transform_attn", "only_area_not_inout")


@pytest.mark.parametrize("member", FAMILY)
@pytest.mark.parametrize("n", [1, 7])
def test_forward_new4_family(member, n):
    """The other New4-family members (model.py:1308-2228), run by the reference with .cuda() as
    the identity (tests/golden/make_golden_new4_family.py)."""
    z = load_golden("new4_family.npz")
    p = params_from(z, member)
    hist, tgt, ref = (z[f"{member}/n{n}/{k}"] for k in ("hist", "target", "pred"))
    got = nais_oracle.forward_family(member, p, z["near"], 32, hist, tgt)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    np.testing.assert_allclose(got[ok], ref[ok], rtol=0, atol=ORACLE_ATOL)


@pytest.mark.parametrize("member", ("New4",) + FAMILY)
@pytest.mark.parametrize("cfg", ["wide", "odd"])
@pytest.mark.parametrize("n", [1, 9])
def test_forward_new4_family_wide(member, cfg, n):
    """All eight table-based members at the reference driver's widths (embed_size = hidden = 128,
    50 near POIs) and at an embed_size off the native widths (48 / 40 / 7), run by the reference
    (tests/golden/make_golden_new4_family_wide.py): pins the oracle at the shapes
    test_gpu_family_shapes.py leans on it for."""
    z = load_golden("new4_family_wide.npz")
    E = int(z[f"{cfg}/shape"][1])
    p = family_wide_params(z, cfg, member)
    hist, tgt, ref = (z[f"{cfg}/{member}/n{n}/{k}"] for k in ("hist", "target", "pred"))
    got = nais_oracle.forward_family(member, p, z[f"{cfg}/near"], E, hist, tgt)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.isnan(ref[0]) == (n == 1)       # the one-item history that is its own target: 0/0
    ok = ~np.isnan(ref)
    np.testing.assert_allclose(got[ok], ref[ok], rtol=0, atol=ORACLE_ATOL)


@pytest.mark.parametrize("member", FAMILY)
def test_catalog_new4_family(member):
    """new4_validation (validation.py:254-280) with each member."""
    z = load_golden("new4_family.npz")
    tag = f"{member}/cat"
    p = params_from(z, tag)
    P, U = int(z["num_pois"]), int(z["num_users"])
    for u in range(U):
        hist = z["indices"][z["indptr"][u]:z["indptr"][u + 1]]
        cand, sc = nais_oracle.catalog_scores_new4(p, z["near_cat"], 32, hist, P, model=member)
        key = f"{tag}/full_scores_u{u}"
        if key in z.files:
            np.testing.assert_allclose(sc, z[key], rtol=0, atol=ORACLE_ATOL)
        ids, top = nais_oracle.topk_ids(cand, sc, 50)
        assert_topk_equivalent(z[f"{tag}/topk_ids"][u], z[f"{tag}/topk_scores"][u], ids, top,
                               tie_ulps=ORACLE_TIE_ULPS, lookup=dict(zip(cand.tolist(), sc.tolist())))


def test_catalog_transform_attn_one_item_histories():
    """transform_attn with 1-item histories: exp_A.squeeze(-1) (model.py:2042) couples the rows of
    each 1024-candidate chunk of new4_validation; the oracle restates the same chunking."""
    z = load_golden("new4_family.npz")
    p = params_from(z, "transform_attn/cat")
    pre = "transform_attn/cat1/"
    indptr, indices = z[pre + "data/indptr"], z[pre + "data/indices"]
    P = int(z[pre + "data/num_pois"])
    for u in range(len(indptr) - 1):
        hist = indices[indptr[u]:indptr[u + 1]]
        cand, sc = nais_oracle.catalog_scores_new4(p, z["near_cat"], 32, hist, P, model="transform_attn")
        np.testing.assert_allclose(sc, z[f"{pre}full_scores_u{u}"], rtol=0, atol=ORACLE_ATOL)


@pytest.mark.parametrize("tag", ["init", "trained"])
@pytest.mark.parametrize("n", [1, 9])
def test_forward_disentangled(tag, n):
    """NAIS_region_distance_disentangled_Embedding (model.py:409-541) run by the reference, with
    run.py:326-333's powerLaw.dist distances (tests/golden/make_golden_disent.py)."""
    from oracle import powerlaw_oracle
    z = load_golden("forward_disent.npz")
    p = params_from(z, tag)
    key = f"{tag}/n{n}"
    hist, tgt, dist, ref = (z[f"{key}/{k}"] for k in ("hist", "target", "dist", "pred"))
    H2 = np.tile(hist, (len(tgt), 1))
    ro = z["region_of"]
    got = nais_oracle._sigmoid(nais_oracle.attention_disentangled(p, H2, tgt, ro[H2], ro[tgt], dist))
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    np.testing.assert_allclose(got[ok], ref[ok], rtol=0, atol=ORACLE_ATOL)
    c = z["coords"]
    mine = np.array([[powerlaw_oracle.dist(c[a], c[h]) for h in hist] for a in tgt], dtype=np.float32)
    assert np.array_equal(mine, dist)


@pytest.mark.parametrize("case", ["region", "region_distance", "basic128", "distance"])
def test_train_oracle_region_variants_match_reference(case):
    """The training restatement for NAIS_regionEmbedding / NAIS_region_distance_Embedding and
    NAIS_basic at run.py's default D = H = 128 vs the reference's autograd
    (tests/golden/make_golden_train_region.py)."""
    from oracle import train_oracle
    z = load_golden("train_step_region.npz")
    pre = case + "/"
    p = {k[len(pre) + 2:]: z[k] for k in z.files if k.startswith(pre + "p/")}
    kw = {}
    if case in ("region", "region_distance"):
        kw.update(hist_region=z[pre + "hist_region"], data_region=z[pre + "data_region"])
    if case in ("region_distance", "distance"):
        kw["latlon"] = z[pre + "latlon"]
    if case == "distance":
        kw["dist_scale"] = 1000.0
    r = train_oracle.train_step(p, z[pre + "hist"], z[pre + "data"], z[pre + "labels"], **kw)
    assert np.max(np.abs(r["pred"] - z[pre + "pred"])) <= 1e-6
    assert abs(r["loss"] - float(z[pre + "loss"])) <= 1e-6
    assert set(r["grads"]) == {k[len(pre) + 5:] for k in z.files if k.startswith(pre + "grad/")}
    for k, g in r["grads"].items():
        ref = z[pre + "grad/" + k]
        assert np.max(np.abs(g.reshape(ref.shape) - ref)) <= 2e-6 * np.abs(ref).max(), k


def test_metric_fixtures_have_no_straddling_ties():
    """The GPU metrics tests (test_gpu_parity.py::_metrics_exact) demand the reference's 6-tuple
    exactly unless a tie run straddles a cut-off k: pin that the golden fixtures hold none, and
    that the 6-tuple restated from the reference's own top-k lists is the captured one."""
    from _helpers import positives_from, straddles
    from oracle import metrics_oracle
    ks = [5, 10, 15, 20, 25, 30]
    for f in ("catalog_basic", "catalog_region", "catalog_distance", "catalog_region_distance"):
        z = load_golden(f + ".npz")
        sc = z["trained/topk_scores"]
        assert not any(straddles(sc[u], k, 4) for u in range(len(sc)) for k in ks), f
        rid = z["trained/topk_ids"].tolist()
        m = metrics_oracle.evaluate(positives_from(z, "val"), rid, ks) + \
            metrics_oracle.evaluate(positives_from(z, "test"), rid, ks)
        np.testing.assert_array_equal(np.array(m), z["trained/metrics"])


def test_new4_metric_fixtures_straddling_ties():
    """The New4 / family metrics tests (test_gpu_parity.py::test_new4_validation_golden,
    test_gpu_family.py::test_family_validation_golden) demand the 6-tuple exactly; pin which
    (user, k) of those fixtures a straddling tie run excuses: none, except New4's "init" tag (the
    reference's N(0, 0.01) init bunches the scores at 0.5), and the captured 6-tuples equal the
    ones restated from the reference's own lists."""
    from _helpers import positives_from, straddles
    from oracle import metrics_oracle
    ks = [5, 10, 15, 20, 25, 30]
    cases = [("new4_catalog", "init"), ("new4_catalog", "trained")] + \
        [("new4_family", n + "/cat") for n in ("New4_padding", "all_in_out", "nearPOI_embedding",
                                               "no_POI_emb", "transform_ingoing_outgoing",
                                               "only_area_not_inout", "transform_attn")]
    for f, tag in cases:
        z = load_golden(f + ".npz")
        sc = z[tag + "/topk_scores"]
        s = [(u, k) for u in range(len(sc)) for k in ks if straddles(sc[u], k, 4)]
        assert s == ([(0, 20), (2, 20), (3, 30), (4, 25), (5, 10)] if tag == "init" else []), (f, tag, s)
        rid = z[tag + "/topk_ids"].tolist()
        m = metrics_oracle.evaluate(positives_from(z, "val"), rid, ks) + \
            metrics_oracle.evaluate(positives_from(z, "test"), rid, ks)
        np.testing.assert_array_equal(np.array(m), z[tag + "/metrics"])
