"""Float64 oracle of one New1 training step (reference run_new.py:403-410, model.py:861-918):
forward, nn.BCELoss, backward, torch.optim.Adam -- and the bound of one fp32 Adam update.

One batch is one user: hist [n] shared by the b target rows. With T / Q the target rows'
concatenated embeddings and attn_Q projections, H / K / V the same for the history and
Ks = the [n, d] key buffer reshaped to [d, n] (model.py:896):

    A = Q Ks / sqrt(d)             E[c][j] = exp(A[c][j]) * [hist_j != target_c]
    S_c = sum_j E[c][j]            M = T V^T           g = sum_j r_j h_j
    N_c = sum_j E[c][j] M[c][j]    pred_c = N_c / S_c^beta + t_c . g,   x_c = sigmoid(pred_c)
    loss = mean_c -(y_c max(log x_c, -100) + (1 - y_c) max(log(1 - x_c), -100))
    d_c  = (x_c - y_c) / max((1 - x_c) x_c, 1e-12) / b * (1 - x_c) x_c
    dM = d E S^-beta,  dA = dM (M - beta N / S),  dQ = dA Ks^T / sqrt(d),  dKs = Q^T dA / sqrt(d)
    dV = dM^T T,  dg = sum_c d_c t_c,  dT = dM V + d g^T + dQ Wq,  dH = dK Wk + dV Wv + r dg^T
    dWq = dQ^T T,  dWk = dK^T H,  dWv = dV^T H;  dT / dH scatter into embed_target / embed_region

d_c is autograd's COMPOSED form (BCELoss's backward, then the sigmoid's), and it depends on how x
rounds in float32: a label-0 row whose x is exactly 1.0f has d = 0, a label-1 row with
x (1 - x) < 1e-12 has |d| = x (1 - x) / 1e-12 / b < 1 / b. So x is rounded to float32 and d_c is
formed in float32 operations, in the order above; everything else is float64.

Adam (torch/optim/adam.py, no amsgrad, not maximize), every element of every tensor:

    g' = g + wd p;  m' = m + (g' - m)(1 - b1);  v' = b2 v + (1 - b2) g'^2
    p' = p - (lr / (1 - b1^t)) m' / (sqrt(v') / sqrt(1 - b2^t) + eps)

The bound of one fp32 update (the second value `adam` returns). Adam's update is normalised, so a gradient error does
not carry into a parameter bound: the optimiser is checked GIVEN the gradients. From the same
float32 p, m, v, g the float64 update above is the exact result; an fp32 evaluation rounds each
operation once (u = 2^-24 relative, fused or not) and holds lr / (1 - b1^t), sqrt(1 - b2^t),
1 - b1, 1 - b2 and b2 as float32 casts of the doubles (u each). To first order:

    dg' <= 2u (|g| + |wd p|)                                  the product and the sum
    dm' <= (1 - b1) dg' + 3u (1 - b1) (|g'| + |m|) + u |m'|   difference, weight cast, product, sum
    dv' <= 2 (1 - b2) |g'| dg' + 4u (1 - b2) g'^2 + 2u b2 v + u v'
    s = sqrt(v') / sqrt(1 - b2^t):   ds <= s (dv' / (2 v') + 3u)      sqrt, the cast, the division
    den = s + eps:                   dden <= ds + u den
    q = m' / den:                    dq <= dm' / den + |q| dden / den + u |q|
    dp' <= step (dq + 2u |q|) + u |p'|                        the step's cast, the product, the sum

plus 2^-126 on each of dm', dv' (a subnormal result may be flushed). The asserted bounds are
ADAM_SLACK = 4 times these first-order terms ("a small multiple"): dp' is a small multiple of
ulp(p) + lr x the ulp-level error of m' / den. tests/test_new1_train_oracle.py asserts that the
reference's own recorded fp32 steps (tests/golden/new1_train.npz) stay inside the bound; the largest
deviation / bound it observes there is ORACLE_DEV_FRACTION.
"""
from __future__ import annotations

import numpy as np

import _new1_oracle as no

NAMES = no.NAMES
U32 = no.U32
ADAM_SLACK = 4.0
# largest |reference fp32 step - this oracle| / adam_bound over every element, tensor and step of
# the fixture (parameters, exp_avg and exp_avg_sq), as test_new1_train_oracle.py prints it
# (0.243, rounded up)
ORACLE_DEV_FRACTION = 0.25
TINY = 2.0 ** -126


def _exp32(a):
    """exp as fp32 sees it: inf above log(FLT_MAX), 0 below half the smallest subnormal."""
    with np.errstate(all="ignore"):
        e = np.where(a > np.log(float(np.finfo(np.float32).max)), np.inf, np.exp(a))
        return np.where(e < 2.0 ** -150, 0.0, e)


def delta32(x32, y, b):
    """d_c in float32 operations from the float32 prediction x (the composed form)."""
    x = np.asarray(x32, dtype=np.float32)
    y = np.asarray(y, dtype=np.float32)
    one = np.float32(1.0)
    with np.errstate(all="ignore"):
        t = (x - y) / np.maximum((one - x) * x, np.float32(1e-12))
        t = t / np.float32(b)
        return (t * (one - x) * x).astype(np.float32)


def step_grads(params, beta, hist, target, labels, hreg, treg, r):
    """(x float64 [b] -- float32 values --, loss, delta [b], {name: dense gradient}) of one batch.
    `r` are the visit rates as the model sees them (float32 values)."""
    Et, Er, Wq, Wk, Wv = (np.asarray(params[k], dtype=np.float64) for k in NAMES)
    hist, target = np.asarray(hist, np.int64), np.asarray(target, np.int64)
    hreg, treg = np.asarray(hreg, np.int64), np.asarray(treg, np.int64)
    y = np.asarray(labels, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    n, b = len(hist), len(target)
    half = Et.shape[1]
    d = 2 * half
    H = np.concatenate([Et[hist], Er[hreg]], -1)
    T = np.concatenate([Et[target], Er[treg]], -1)
    Q, K, V = T @ Wq.T, H @ Wk.T, H @ Wv.T
    Ks = K.reshape(d, n)
    sqd = np.sqrt(float(d))
    with np.errstate(all="ignore"):
        A = (Q @ Ks) / sqd
        E = _exp32(A) * (hist[None, :] != target[:, None])
        S = E.sum(1)
        M = T @ V.T
        g = r @ H
        N = (E * M).sum(1)
        Sp = S ** (-beta)
        pred = N * Sp + T @ g
        # 1 / (1 + exp(-pred)) in float32 operations: exactly 0 once exp(-pred) overflows, exactly
        # 1 once 1 + exp(-pred) rounds to 1
        x = np.float32(1.0) / (np.float32(1.0) + _exp32(-pred).astype(np.float32))
        x64 = x.astype(np.float64)
        lt = -(y * np.maximum(np.log(x64), -100.0) + (1.0 - y) * np.maximum(np.log1p(-x64), -100.0))
        loss = float(lt.mean())
        dl = delta32(x, y, b).astype(np.float64)
        dM = dl[:, None] * E * Sp[:, None]
        dA = dM * (M - (beta * N / S)[:, None]) / sqd
        dQ = dA @ Ks.T
        dK = (Q.T @ dA).reshape(n, d)
        dV = dM.T @ T
        dg = dl @ T
        dT = dM @ V + np.outer(dl, g) + dQ @ Wq
        dH = dK @ Wk + dV @ Wv + np.outer(r, dg)
    grads = {NAMES[0]: np.zeros_like(Et), NAMES[1]: np.zeros_like(Er),
             NAMES[2]: dQ.T @ T, NAMES[3]: dK.T @ H, NAMES[4]: dV.T @ H}
    np.add.at(grads[NAMES[0]], target, dT[:, :half])
    np.add.at(grads[NAMES[0]], hist, dH[:, :half])
    np.add.at(grads[NAMES[1]], treg, dT[:, half:])
    np.add.at(grads[NAMES[1]], hreg, dH[:, half:])
    return x64, loss, dl, grads


def adam(p, m, v, g, t, lr, wd, betas=(0.9, 0.999), eps=1e-8, with_bound=True):
    """One Adam update of one tensor in float64 from float32 p, m, v, g. Returns (p', m', v') and,
    with_bound, the bounds (dp', dm', dv') of an fp32 evaluation (module docstring)."""
    p, m, v, g = (np.asarray(a, dtype=np.float64) for a in (p, m, v, g))
    b1, b2 = betas
    gp = g + wd * p
    m2 = m + (gp - m) * (1.0 - b1)
    v2 = b2 * v + (1.0 - b2) * gp * gp
    step = lr / (1.0 - b1 ** t)
    bc2 = np.sqrt(1.0 - b2 ** t)
    s = np.sqrt(v2) / bc2
    den = s + eps
    q = m2 / den
    p2 = p - step * q
    if not with_bound:
        return (p2, m2, v2), None
    u = U32
    dg = 2 * u * (np.abs(g) + np.abs(wd * p))
    dm = (1 - b1) * dg + 3 * u * (1 - b1) * (np.abs(gp) + np.abs(m)) + u * np.abs(m2) + TINY
    dv = 2 * (1 - b2) * np.abs(gp) * dg + 4 * u * (1 - b2) * gp * gp + 2 * u * b2 * v + u * v2 + TINY
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(v2 > 0, dv / (2 * v2), 0.0)
    # v' = 0 only where g' = 0 and v = 0: then s = 0 exactly and sqrt(dv') bounds it
    ds = np.where(v2 > 0, s * (rel + 3 * u), np.sqrt(dv) / bc2)
    dden = ds + u * den
    dq = dm / den + np.abs(q) * dden / den + u * np.abs(q)
    dp = step * (dq + 2 * u * np.abs(q)) + u * np.abs(p2)
    return (p2, m2, v2), (ADAM_SLACK * dp, ADAM_SLACK * dm, ADAM_SLACK * dv)


def adam_all(params, exp_avg, exp_avg_sq, grads, t, lr, wd, betas=(0.9, 0.999), eps=1e-8):
    """adam() over the five tensors: ({name: (p', m', v')}, {name: (dp', dm', dv')})."""
    out, bnd = {}, {}
    for k in NAMES:
        out[k], bnd[k] = adam(params[k], exp_avg[k], exp_avg_sq[k], grads[k], t, lr, wd, betas, eps)
    return out, bnd
