"""Float64 numpy restatement of BPR (model.py:587-620, validation.py:133-153, run.py:504-509):
scores, top-k, loss, gradients and the SGD step. Test infrastructure only.

`E(U, I)` is the score tolerance. A length-D fp32 dot product summed in any order is within
gamma_D * sum_e |u_e i_e| of the exact value, gamma_D <= (D + 1) * 2^-24 for D <= 256; two such
results (ours and the reference's) are compared, hence
    E(u, c) = 2 * (D + 1) * 2^-24 * sum_e |U[u, e] * I[c, e]|        (the sum in float64).
"""
from __future__ import annotations

import numpy as np


def scores(U, I):
    """[users, P] float64 inner products."""
    return np.asarray(U, np.float64) @ np.asarray(I, np.float64).T


def E(U, I):
    """[users, P] float64 tolerance of one fp32 score against another (module docstring)."""
    U, I = np.asarray(U, np.float64), np.asarray(I, np.float64)
    return 2.0 * (U.shape[1] + 1) * 2.0 ** -24 * (np.abs(U) @ np.abs(I).T)


def topk(row, hist, k):
    """(ids, scores) of the k best candidates of [0, P) minus `hist`: score descending, NaN first
    (torch.topk's rank of NaN), ties by ascending id. Fewer than k candidates: a shorter list."""
    row = np.asarray(row, np.float64)
    cand = np.setdiff1d(np.arange(len(row)), np.asarray(hist, np.int64))
    s = row[cand]
    rank = np.where(np.isnan(s), np.inf, s)
    order = np.lexsort((cand, -rank))[:k]
    return cand[order], s[order]


def step(U, I, user, item_i, item_j, lr, weight_decay=0.0):
    """One run.py:504-509 step. Returns dict(loss, pred_i, pred_j, g, grad_user, grad_item,
    embed_user, embed_item) in float64. The sigmoid is rounded to float32 as the reference
    computes it, so a saturated s == 0 gives its inf loss and NaN gradient; g is autograd's
    composed form (-1 / s) * ((1 - s) * s)."""
    U, I = np.asarray(U, np.float64), np.asarray(I, np.float64)
    user, item_i, item_j = (np.asarray(a, np.int64) for a in (user, item_i, item_j))
    pi = np.sum(U[user] * I[item_i], -1)
    pj = np.sum(U[user] * I[item_j], -1)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        x = (pi - pj).astype(np.float32)
        s = (np.float32(1) / (np.float32(1) + np.exp(-x))).astype(np.float64)
        loss = -np.sum(np.log(s))
        g = (-1.0 / s) * ((1.0 - s) * s)
        gu, gi = np.zeros_like(U), np.zeros_like(I)
        np.add.at(gu, user, g[:, None] * (I[item_i] - I[item_j]))
        np.add.at(gi, item_i, g[:, None] * U[user])
        np.add.at(gi, item_j, -g[:, None] * U[user])
        nu = U - lr * (gu + weight_decay * U)
        ni = I - lr * (gi + weight_decay * I)
    return dict(loss=loss, pred_i=pi, pred_j=pj, g=g, grad_user=gu, grad_item=gi, embed_user=nu,
                embed_item=ni)


def post_step_table(z, tag, name, key):
    """The reference's table `key` after the fixture's training step of `tag` at weight decay
    `name`, whole. At weight decay 0 the fixture stores the touched rows only (the capture script
    asserts that no other row moved): they are put back into the pre-step table."""
    pre = f"{tag}/train/{name}/"
    if pre + "rows/" + key not in z.files:
        return z[pre + key]
    full = z[f"{tag}/{key}"].copy()
    full[z[pre + "rows/" + key]] = z[pre + key]
    return full
