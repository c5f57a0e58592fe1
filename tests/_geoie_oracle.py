"""numpy fp32 restatement of the reference's GeoIE (model.py:757-828) and of its evaluation loop
(validation.py:183-195 with get_GeoIE_batch_test, batches.py:244-269). Test infrastructure only:
nothing under poi_recommendation_models_amd/ imports it.
"""
from __future__ import annotations

import numpy as np

from oracle import powerlaw_oracle

# Largest fp32-ulp distance between the reference's and this oracle's scores over every catalog
# row of tests/golden/geoie.npz (tests/test_geoie_oracle.py measures it and asserts this value),
# and the tie window of every GeoIE top-k comparison: the project's 4 ulps, or twice M because the
# GPU is a third fp32 implementation that may sit M on the other side of the reference.
M_ULPS = 3
TIE_ULPS = max(4, 2 * M_ULPS)


def clamped_dist(c1, c2):
    """run.py:44: min(max(0.01, dist(poi_coos[i], poi_coos[j])), 100), float64."""
    return min(max(0.01, powerlaw_oracle.dist(c1, c2)), 100)


def distance_mat(coords):
    """run.distance_mat (run.py:40-46): the P x P float64 matrix the reference unpickles at :683."""
    P = len(coords)
    cs = [tuple(float(v) for v in c) for c in coords]
    out = np.zeros([P, P])
    for i in range(P):
        for j in range(P):
            out[i][j] = clamped_dist(cs[i], cs[j])
    return out


def distance_rows(coords, targets, hist):
    """float32 [len(targets), h]: dist_mat[t, hist] (batches.py:256, :267) without the matrix."""
    cs = [tuple(float(v) for v in c) for c in coords]
    return np.array([[clamped_dist(cs[int(t)], cs[int(j)]) for j in hist] for t in targets],
                    dtype=np.float64).astype(np.float32)


def wuj(freq, scaling=10):
    """model.py:812: 1 + log(1 + cuj * 10**scaling); the log of an int64 tensor is float32."""
    x = (1 + np.asarray(freq, dtype=np.int64) * (10 ** scaling)).astype(np.float32)
    return (np.float32(1) + np.log(x)).astype(np.float32)


def forward(p, a, b, user, targets, hist, dist, chunk=64):
    """prediction [b] float32 for rows that share ONE history `hist` [h] (every batch the
    reference builds does, batches.py:211, :251); dist [b, h] float32. model.py:785-813."""
    f32 = np.float32
    hist = np.asarray(hist, dtype=np.int64)
    targets = np.asarray(targets, dtype=np.int64)
    h, D = len(hist), p["GeoInfluence.weight"].shape[1]
    if h == 0:
        raise ValueError("empty history")
    # g.reshape([b, -1, h]) of the [h, D] gather: a reinterpretation, not a transpose (model.py:798)
    Gr = p["GeoInfluence.weight"][hist].astype(f32).reshape(-1).reshape(D, h)
    fij = f32(a) * np.power(np.asarray(dist, dtype=f32), f32(b))            # model.py:799
    up = p["UserPreference.weight"][np.asarray(user, dtype=np.int64)].astype(f32)
    out = np.empty(len(targets), dtype=f32)
    for s in range(0, len(targets), chunk):
        t = targets[s:s + chunk]
        hj = p["GeoSusceptibility.weight"][t].astype(f32)                   # [c, D]
        t1 = Gr[None, :, :] * hj[:, :, None]                                # model.py:801
        t2 = t1.sum(axis=1, dtype=f32) * fij[s:s + chunk]                   # model.py:802
        yij = t2.sum(axis=-1, dtype=f32) / f32(h)                           # model.py:803
        tz = (up[s:s + chunk] * p["PoiPreference.weight"][t].astype(f32)).sum(axis=-1, dtype=f32)
        suj = (tz + yij).astype(f32)                                        # model.py:810
        with np.errstate(over="ignore"):
            out[s:s + chunk] = f32(1) / (f32(1) + np.exp(-suj, dtype=f32))
    return out


def catalog_scores(p, a, b, u, hist, P, coords=None, dist_mat=None):
    """(candidates int64 ascending, scores f32): get_GeoIE_batch_test's complement of the history
    (batches.py:250) scored with freq = 1, as validation.py:188-189."""
    hist = np.asarray(hist, dtype=np.int64)
    cand = np.setdiff1d(np.arange(P, dtype=np.int64), hist)
    if dist_mat is not None:
        dist = np.asarray(dist_mat)[cand][:, hist].astype(np.float32)
    else:
        dist = distance_rows(coords, cand, hist)
    return cand, forward(p, a, b, np.full(len(cand), u, dtype=np.int64), cand, hist, dist)


def topk(cand, scores, k):
    """torch.topk(prediction.squeeze(), k) (validation.py:190): descending, NaN first; ties by
    ascending candidate (one valid order of torch's unspecified tie order)."""
    if k > len(cand):
        raise RuntimeError("selected index k out of range")
    key = np.where(np.isnan(scores), np.inf, scores.astype(np.float64))
    order = np.lexsort((cand, -key))[:k]
    return cand[order], scores[order]


def loss_function(prediction, label, weight):
    """model.py:816-828, float32."""
    f32 = np.float32
    pr = np.asarray(prediction, dtype=f32)
    lb = np.asarray(label, dtype=f32)
    t1 = lb * np.log(pr + f32(1e-10))
    t2 = (f32(1) - lb) * np.log(f32(1) - pr + f32(1e-10))
    return np.sum(-np.asarray(weight, dtype=f32) * (t1 + t2), dtype=f32)


PARAM_NAMES = ("UserPreference.weight", "PoiPreference.weight", "GeoInfluence.weight",
               "GeoSusceptibility.weight")
_fixture = {}


def fixture():
    """tests/golden/geoie.npz with what every test derives from it, computed once and shared:
    the rebuilt dist_mat, per-tag parameters / (a, b), and the oracle's own catalog rows."""
    if _fixture:
        return _fixture
    from _helpers import load_golden, positives_from
    z = load_golden("geoie.npz")
    P, U = int(z["num_pois"]), int(z["num_users"])
    fx = dict(z=z, P=P, U=U, D=int(z["embed_dim"]), coords=z["coords"], indptr=z["indptr"],
              indices=z["indices"], k_list=[int(k) for k in z["k_list"]],
              val=positives_from(z, "val"), test=positives_from(z, "test"),
              dist_mat=distance_mat(z["coords"]), tags={})
    for tag in ("init", "spread"):
        p = {n: z[f"{tag}/{n}"] for n in PARAM_NAMES}
        a, b = (float(v) for v in z[f"{tag}/ab"])
        rows = np.full((U, P), -1.0, dtype=np.float32)
        for u in range(U):
            hist = fx["indices"][fx["indptr"][u]:fx["indptr"][u + 1]]
            cand, sc = catalog_scores(p, a, b, u, hist, P, dist_mat=fx["dist_mat"])
            rows[u, cand] = sc
        rows.setflags(write=False)
        fx["tags"][tag] = dict(p=p, a=a, b=b, rows=rows)
    _fixture.update(fx)
    return _fixture


def history(fx, u):
    return fx["indices"][fx["indptr"][u]:fx["indptr"][u + 1]]


def train_matrix(fx):
    import scipy.sparse as sp
    return sp.csr_matrix((fx["z"]["data"], fx["indices"], fx["indptr"]), shape=(fx["U"], fx["P"]))


def ulp_distance(x, y):
    """fp32 ulps between x and y (elementwise; both finite, same sign or zero)."""
    a = np.asarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(y, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)
