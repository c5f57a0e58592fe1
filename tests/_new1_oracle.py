"""Float64 oracle of the New1 model (reference model.py:830-925) and the tolerance E of one fp32
evaluation against exact arithmetic.

The model. Parameters are the state_dict arrays (`embed_target.weight [P, d/2]`,
`embed_region.weight [R, d/2]`, `attn_Q.weight`, `attn_K.weight`, `attn_V.weight`, each [d, d]).
With h_j = [Et[hist_j] | Er[hreg_j]], t = [Et[c] | Er[treg]], q = Wq t, K_j = Wk h_j, V_j = Wv h_j:

    M      = the [n, d] buffer (K_j[k]) RESHAPED to [d, n] (model.py:896; not a transpose)
    a_j    = (sum_e q_e M[e, j]) / sqrt(d)
    e_j    = exp(a_j) * [hist_j != c]
    S      = sum_j e_j,   w_j = e_j / S^beta
    pred   = sum_j sum_k (w_j V_jk + r_j h_jk) t_k,   score = sigmoid(pred)

An empty history is pred = 0 (score 0.5); n = 1 is this formula (the reference's squeeze() calls
mix the rows of the batch there). `transposed=True` replaces the reshape by a plain transpose: the
variant the fixture must NOT match.

The bound E(u, c). u = 2^-24 is fp32's unit roundoff and gamma_m = m u / (1 - m u) the usual
bound of an m-term fp32 sum or dot product in any order. The parameters are fp32 numbers, so the
exact model is evaluated on exactly the inputs the fp32 code sees; E bounds, to first order, the
distance of any fp32 evaluation of the formula above from it, each elementary function (exp, pow,
the sigmoid's exp) within 2u relative, division, sqrt and the basic operations correctly
rounded. All quantities below are computed in float64 from absolute values:

    dq_e    <= gamma_d (|Wq| |t|)_e                       the projections: length-d dots
    dK_jk   <= gamma_d (|Wk| |h_j|)_k  (dM the same, reshaped),   dV_jk <= gamma_d (|Wv| |h_j|)_k
    da_j    <= [gamma_d (|q| |M|)_j + (dq |M|)_j + (|q| dM)_j] / sqrt(d) + 2u |a_j|
               the length-d dot of computed operands, then sqrt and the division (u each)
    ee_j    =  expm1(da_j) + 2u                           relative error of e_j
    eS      =  (sum_j e_j ee_j) / S + gamma_n             relative error of S
    ep      =  beta eS + 2u                               relative error of S^beta
    ew_j    =  ee_j + ep + u                              relative error of w_j
    dpred   <= sum_jk |w_j V_jk t_k| (ew_j + 4u)          w's error, the products' roundings
             + sum_jk w_j dV_jk |t_k|                     V's error
             + 3u sum_jk |r_j h_jk t_k|                   the visit-rate term's roundings
             + gamma_{n+d} sum_jk |(w_j V_jk + r_j h_jk) t_k|    the final double sum, any order
    E       =  dpred / 4 + 2u

The last line: sigmoid is 1/4-Lipschitz; computed as 1 / (1 + exp(-x)) its own roundings cost at
most (2 s (1 - s) + 2 s) u <= 2u at s = sigmoid(x) (exp within 2u relative, the addition and the
division correctly rounded). A factorised evaluation (sum_j e_j (V_j . t) divided by S^beta, plus
t . sum_j r_j h_j, as the catalog scorer computes it) performs the same operations regrouped and
is covered by the same first-order terms. Two fp32 results (ours and the reference's) are
compared at 2E, one result against this oracle at E. E is NaN / inf exactly where the score is
NaN (overflow, S = 0); those rows are compared by their NaN pattern.
"""
from __future__ import annotations

import numpy as np

U32 = 2.0 ** -24
NAMES = ("embed_target.weight", "embed_region.weight", "attn_Q.weight", "attn_K.weight",
         "attn_V.weight")


def gamma(m):
    return m * U32 / (1.0 - m * U32)


def _f64(params):
    return [np.asarray(params[k], dtype=np.float64) for k in NAMES]


def rows_of(params, ids, regions):
    """Concatenated rows [Et[id] | Er[region]] in float64."""
    Et, Er = _f64(params)[:2]
    return np.concatenate([Et[np.asarray(ids)], Er[np.asarray(regions)]], axis=-1)


def score_user(params, beta, hist, hreg, r, cands, cregs, transposed=False, with_E=True):
    """Scores (float64 [C]) of candidates `cands` (regions `cregs`) against ONE history (`hist`,
    `hreg`, visit rates `r`), and E per candidate (None when with_E is False)."""
    _, _, Wq, Wk, Wv = _f64(params)
    hist, cands = np.asarray(hist, dtype=np.int64), np.asarray(cands, dtype=np.int64)
    n, C = len(hist), len(cands)
    d = Wq.shape[1]
    if n == 0:
        return np.full(C, 0.5), (np.full(C, 2 * U32) if with_E else None)
    h = rows_of(params, hist, hreg)
    t = rows_of(params, cands, cregs)
    r = np.asarray(r, dtype=np.float64)
    q = t @ Wq.T
    Kf = h @ Wk.T
    M = Kf.T if transposed else Kf.reshape(d, n)
    Vv = h @ Wv.T
    with np.errstate(all="ignore"):
        a = (q @ M) / np.sqrt(float(d))
        mask = hist[None, :] != cands[:, None]
        # exp as fp32 sees it: inf above log(FLT_MAX), 0 below half the smallest subnormal; the
        # mask is a product, so inf * 0 = NaN (model.py:899-901)
        e = np.where(a > np.log(float(np.finfo(np.float32).max)), np.inf, np.exp(a))
        e = np.where(e < 2.0 ** -150, 0.0, e) * mask.astype(np.float64)
        S = e.sum(1)
        w = e / (S ** beta)[:, None]
        vt = t @ Vv.T
        g = r @ h
        pred = (w * vt).sum(1) + t @ g
        score = 1.0 / (1.0 + np.exp(-pred))
        if not with_E:
            return score, None
        gd, gn, gnd = gamma(d), gamma(n), gamma(n + d)
        at, aq = np.abs(t), np.abs(q)
        dq = gd * (at @ np.abs(Wq).T)
        dK = gd * (np.abs(h) @ np.abs(Wk).T)
        dM = dK.T if transposed else dK.reshape(d, n)
        aM = np.abs(M)
        da = (gd * (aq @ aM) + dq @ aM + aq @ dM) / np.sqrt(float(d)) + 2 * U32 * np.abs(a)
        ee = np.expm1(da) + 2 * U32
        eS = (e * ee).sum(1) / S + gn
        ep = beta * eS + 2 * U32
        ew = ee + ep[:, None] + U32
        avt = at @ np.abs(Vv).T
        dV = gd * (np.abs(h) @ np.abs(Wv).T)
        ag = at @ (np.abs(r) @ np.abs(h))
        dpred = ((w * (ew + 4 * U32) * avt).sum(1) + (w * (at @ dV.T)).sum(1) + 3 * U32 * ag
                 + gnd * ((w * avt).sum(1) + ag))
        E = dpred / 4.0 + 2 * U32
    return score, E


def logits(params, hist, hreg, cands, cregs):
    """a [C, n] of the formula above (float64), for choosing overflow cases."""
    _, _, Wq, Wk, _ = _f64(params)
    d, n = Wq.shape[1], len(hist)
    q = rows_of(params, cands, cregs) @ Wq.T
    return (q @ (rows_of(params, hist, hreg) @ Wk.T).reshape(d, n)) / np.sqrt(float(d))


def forward_rows(params, beta, hist, target, hreg, treg, r, transposed=False):
    """The batch forward: rows with their own histories ([b, n] arrays). (scores, E) float64 [b]."""
    hist, hreg = np.asarray(hist), np.asarray(hreg)
    out, tol = [], []
    for i in range(hist.shape[0]):
        s, E = score_user(params, beta, hist[i], hreg[i], r, [int(target[i])], [int(treg[i])],
                          transposed)
        out.append(s[0])
        tol.append(E[0])
    return np.array(out), np.array(tol)


def visit_rates(indptr, indices, data, num_pois):
    """r per CSR entry: data / colsum[indices] in float64 (batches.py:350-359)."""
    colsum = np.zeros(num_pois, dtype=np.float64)
    np.add.at(colsum, indices, np.asarray(data, dtype=np.float64))
    return np.asarray(data, dtype=np.float64) / colsum[indices]


def user_row(params, beta, indptr, indices, rate, region_of, u, with_E=True):
    """(candidates ascending, scores, E) of user u over [0, P) minus its history."""
    P = np.asarray(params[NAMES[0]]).shape[0]
    region_of = np.asarray(region_of)
    hist = np.asarray(indices[indptr[u]:indptr[u + 1]], dtype=np.int64)
    cands = np.setdiff1d(np.arange(P, dtype=np.int64), hist)
    s, E = score_user(params, beta, hist, region_of[hist], rate[indptr[u]:indptr[u + 1]], cands,
                      region_of[cands], with_E=with_E)
    return cands, s, E


def topk(cands, scores, k):
    """The selection on the scores: descending, NaN first (as torch.topk ranks it), ties by
    ascending POI id. Returns (ids, scores) of min(k, len) entries."""
    s = np.asarray(scores, dtype=np.float64)
    key = np.where(np.isnan(s), np.inf, s)
    order = np.lexsort((np.asarray(cands), -key))[:k]
    return np.asarray(cands)[order], s[order]
