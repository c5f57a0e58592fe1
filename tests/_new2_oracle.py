"""Float64 oracle of the New2 model (reference model.py:927-1027) and the tolerance E of one fp32
evaluation against exact arithmetic. It extends tests/_new1_oracle.py (same symbols, same u and
gamma_m); read that docstring first.

The model. Parameters are New1's state_dict arrays plus `embed_dist [U, R]`. For a batch of b rows
with n history items each, w = embed_dist[uid], dist the [n, b] block (history rows x target
columns) the dataset hands over, flattened:

    tau_c     = w[treg_c],   omega_cj = w[hreg_cj]
    G_j       = sum_c tau_c omega_cj              over THE BATCH: one vector for every row
    lambda_j  = -1 / (relu(G_j) + 1)
    D'_cj     = distflat[c n + j]                 a RESHAPE of [n, b] to [b, n], not a transpose
    geo_cj    = exp(lambda_j D'_cj)               (not masked)
    pred_c    = sum_j (w_cj + geo_cj) (V_j . t_c) + t_c . sum_j r_j h_j,   score = sigmoid(pred)

with w_cj New1's attention weight e_cj / S_c^beta. Two variants the fixture must NOT match:
`dist_transposed=True` reads D'_cj = dist[j][c] (the block transposed instead of reshaped) and
`per_row_G=True` uses G_cj = tau_c omega_cj (no sum over the batch).

The bound E extends New1's (all quantities in float64 from absolute values):

    dG_j   <= gamma_b sum_c |tau_c omega_cj|      a b-term sum of products, any order; the scorer's
                                                  G_j = omega_j * fl(sigma_u), sigma_u summed in
                                                  float64 and rounded once, is two roundings
    s_j     = relu(G_j) + 1 >= 1:  ds_j <= dG_j + u s_j         relu is 1-Lipschitz; the addition
    lambda_j = -1 / s_j:  relative ds_j / s_j + u
    D'_cj:  relative 2u = 2^-23                   the cast to float32 is u; a few float64 ulps of
                                                  libm error in the distance can move the rounding
                                                  by at most one step
    x_cj    = lambda_j D'_cj:  dx <= |x| (ds_j / s_j + 4u)
    eg_cj   = expm1(dx_cj) + 2u                   relative error of geo (expf within 2u), plus
                                                  2^-126 absolute where the result is subnormal
    dpred  <= New1's terms with w + geo in place of w in the V-error and final-sum terms,
              + sum_j geo_cj (eg_cj + 5u) |V_j|.|t_c|           geo's error, the addition w + geo,
                                                                 the products' roundings
              + gamma_n sum_j |(w + geo)_cj| |V_j|.|t_c|        one more n-term sum
    E       = dpred / 4 + 2u

One fp32 result is compared against this oracle at E, two fp32 results at 2E. E is NaN / inf
exactly where the score is NaN.
"""
from __future__ import annotations

import numpy as np

from _new1_oracle import U32, gamma, topk  # noqa: F401  (topk: the selection rule, shared)

NAMES = ("embed_target.weight", "embed_region.weight", "attn_Q.weight", "attn_K.weight",
         "attn_V.weight", "embed_dist")
EARTH_RADIUS_KM = 6371.0088


def haversine_km(a, b):
    """[len(a), len(b)] float64 kilometres: haversine_vector(a, b, comb=True)'s formula."""
    a, b = np.radians(np.asarray(a, np.float64)), np.radians(np.asarray(b, np.float64))
    lat = b[None, :, 0] - a[:, None, 0]
    lng = b[None, :, 1] - a[:, None, 1]
    d = np.sin(lat * 0.5) ** 2 + np.cos(a[:, None, 0]) * np.cos(b[None, :, 0]) * np.sin(lng * 0.5) ** 2
    return 2 * EARTH_RADIUS_KM * np.arcsin(np.sqrt(d))


def score_rows(params, beta, hist, hreg, r, target, treg, dist, uid, transposed=False,
               dist_transposed=False, per_row_G=False, with_E=True):
    """(scores, E) float64 [b] of a batch: hist / hreg [b, n] (rows may be broadcast views),
    r [n], target / treg [b], dist with n * b elements (the [n, b] block, any shape; its values are
    taken as the float32 numbers they are cast to)."""
    Et, Er, Wq, Wk, Wv, Wd = [np.asarray(params[k], dtype=np.float64) for k in NAMES]
    hist, hreg = np.asarray(hist, dtype=np.int64), np.asarray(hreg, dtype=np.int64)
    target, treg = np.asarray(target, dtype=np.int64), np.asarray(treg, dtype=np.int64)
    b, n = hist.shape
    d = Wq.shape[1]
    if n == 0:
        return np.full(b, 0.5), (np.full(b, 2 * U32) if with_E else None)
    dist = np.asarray(dist, dtype=np.float32).astype(np.float64)
    assert dist.size == n * b
    D = dist.reshape(n, b).T if dist_transposed else dist.reshape(b, n)
    h = np.concatenate([Et[hist], Er[hreg]], axis=-1)                  # [b, n, d]
    t = np.concatenate([Et[target], Er[treg]], axis=-1)                # [b, d]
    r = np.asarray(r, dtype=np.float64)
    q = t @ Wq.T
    Kf = h @ Wk.T
    M = Kf.transpose(0, 2, 1) if transposed else Kf.reshape(b, d, n)
    Vv = h @ Wv.T
    wu = Wd[int(uid)]
    tau, om = wu[treg], wu[hreg]
    with np.errstate(all="ignore"):
        a = np.einsum("be,bej->bj", q, M) / np.sqrt(float(d))
        mask = hist != target[:, None]
        e = np.where(a > np.log(float(np.finfo(np.float32).max)), np.inf, np.exp(a))
        e = np.where(e < 2.0 ** -150, 0.0, e) * mask.astype(np.float64)
        S = e.sum(1)
        w = e / (S ** beta)[:, None]
        prod = tau[:, None] * om                                       # [b, n]
        G = prod if per_row_G else np.broadcast_to(prod.sum(0), (b, n))
        s = np.maximum(G, 0.0) + 1.0
        x = -1.0 / s * D
        geo = np.exp(x)
        geo = np.where(geo < 2.0 ** -150, 0.0, geo)
        vt = np.einsum("bnd,bd->bn", Vv, t)
        ht = np.einsum("bnd,bd->bn", h, t)
        pred = ((w + geo) * vt).sum(1) + (ht * r[None, :]).sum(1)
        score = 1.0 / (1.0 + np.exp(-pred))
        if not with_E:
            return score, None
        gd, gn, gnd = gamma(d), gamma(n), gamma(n + d)
        at, aq, ah = np.abs(t), np.abs(q), np.abs(h)
        dq = gd * (at @ np.abs(Wq).T)
        dK = gd * (ah @ np.abs(Wk).T)
        dM = dK.transpose(0, 2, 1) if transposed else dK.reshape(b, d, n)
        aM = np.abs(M)
        da = (gd * np.einsum("be,bej->bj", aq, aM) + np.einsum("be,bej->bj", dq, aM)
              + np.einsum("be,bej->bj", aq, dM)) / np.sqrt(float(d)) + 2 * U32 * np.abs(a)
        ee = np.expm1(da) + 2 * U32
        eS = (e * ee).sum(1) / S + gn
        ep = beta * eS + 2 * U32
        ew = ee + ep[:, None] + U32
        avt = np.einsum("bnd,bd->bn", np.abs(Vv), at)
        dV = gd * (ah @ np.abs(Wv).T)
        dvt = np.einsum("bnd,bd->bn", dV, at)
        ag = (np.einsum("bnd,bd->bn", ah, at) * np.abs(r)[None, :]).sum(1)
        aprod = np.abs(prod)
        dG = (gamma(1) * aprod) if per_row_G else np.broadcast_to(gamma(b) * aprod.sum(0), (b, n))
        ds = dG + U32 * s
        dx = np.abs(x) * (ds / s + 4 * U32)
        eg = np.expm1(dx) + 2 * U32
        wg = w + geo
        dpred = ((w * (ew + 5 * U32) * avt).sum(1) + (geo * (eg + 5 * U32) * avt).sum(1)
                 + 2.0 ** -126 * avt.sum(1) + (wg * dvt).sum(1) + 3 * U32 * ag
                 + (gnd + gn) * ((wg * avt).sum(1) + ag))
        E = dpred / 4.0 + 2 * U32
    return score, E


def geo_terms(params, hreg, treg, dist, uid):
    """(G [n], geo [b, n]) of a batch in float64: for choosing and checking fixture cases."""
    wu = np.asarray(params["embed_dist"], dtype=np.float64)[int(uid)]
    hreg, treg = np.asarray(hreg), np.asarray(treg)
    b, n = hreg.shape
    G = (wu[treg][:, None] * wu[hreg]).sum(0)
    D = np.asarray(dist, dtype=np.float32).astype(np.float64).reshape(b, n)
    return G, np.exp(-1.0 / (np.maximum(G, 0.0) + 1.0) * D)


def user_row(params, beta, indptr, indices, rate, region_of, dist32, u, with_E=True, **variant):
    """(candidates ascending, scores, E) of user u as the reference's evaluation batch
    (testDataset2.__getitem__, run_new.py:242-264): every POI outside the history in ascending id,
    one shared history, the block dist32[history][:, candidates] ([n, b]) and uid = u."""
    P = np.asarray(params[NAMES[0]]).shape[0]
    region_of = np.asarray(region_of)
    hist = np.asarray(indices[indptr[u]:indptr[u + 1]], dtype=np.int64)
    cands = np.setdiff1d(np.arange(P, dtype=np.int64), hist)
    b, n = len(cands), len(hist)
    block = np.asarray(dist32)[hist][:, cands]
    s, E = score_rows(params, beta, np.broadcast_to(hist, (b, n)),
                      np.broadcast_to(region_of[hist], (b, n)), rate[indptr[u]:indptr[u + 1]],
                      cands, region_of[cands], block, u, with_E=with_E, **variant)
    return cands, s, E
