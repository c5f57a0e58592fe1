"""numpy fp32 restatement of one train_GeoIE step (run.py:705-715: model.py:785-828 forward,
loss_function, autograd's backward, torch.optim.SGD without momentum). Test infrastructure only.

The summation order differs from torch's and from the kernels' on purpose: the two products are
fp32 BLAS matmuls of T = F . Gr^T first (torch sums over e first, then j; the kernels chain fmafs
in k order), and the loss is a pairwise numpy sum.
"""
from __future__ import annotations

import numpy as np

import _geoie_oracle as go

PARAM_NAMES = go.PARAM_NAMES
f32 = np.float32

# Largest deviation of this oracle's parameters from the reference's after the three-step
# trajectories of tests/golden/geoie_train.npz, as a fraction of the trajectory tolerance
# TRAJ_STEPS * (lr * GRAD_RTOL * max|g| + 2 ulp(p)) (tests/test_geoie_train_oracle.py measures it
# and asserts this bound). Below 1/2, so the GPU tests keep the issue's tolerance as it stands.
ORACLE_DEV_FRACTION = 0.002   # measured 0.0018
TRAJ_STEPS = 3


def step_grads(p, a, b, user, hist, target, label, freq, dist):
    """Forward, loss and row gradients of one batch (one user, one shared history).
    Returns dict(pred [b], score [b] (the logit), loss f32, terms [b], delta [b], grads {name: rows in batch order})."""
    hist = np.asarray(hist, dtype=np.int64).reshape(-1)
    target = np.asarray(target, dtype=np.int64).reshape(-1)
    label = np.asarray(label, dtype=f32).reshape(-1)
    h, D = len(hist), p["GeoInfluence.weight"].shape[1]
    if h == 0:
        raise ValueError("empty history")
    Gr = p["GeoInfluence.weight"][hist].astype(f32).reshape(-1).reshape(D, h)   # model.py:798
    F = (f32(a) * np.power(np.asarray(dist, dtype=f32), f32(b))).astype(f32)     # [b, h]
    Hs = p["GeoSusceptibility.weight"][target].astype(f32)
    Pp = p["PoiPreference.weight"][target].astype(f32)
    up = p["UserPreference.weight"][int(user)].astype(f32)
    T = (F @ Gr.T).astype(f32)                                                   # [b, D]
    y = (T * Hs).sum(axis=1, dtype=f32) / f32(h)
    tz = (Pp @ up).astype(f32)
    s = (tz + y).astype(f32)
    with np.errstate(over="ignore"):
        pr = (f32(1) / (f32(1) + np.exp(-s, dtype=f32))).astype(f32)
    w = go.wuj(np.asarray(freq).reshape(-1))
    eps = f32(1e-10)
    q = (f32(1) - pr).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = (-w * (label * np.log(pr + eps) + (f32(1) - label) * np.log(q + eps))).astype(f32)
        # autograd's composed form (exactly 0 where p rounds to 0 or 1), not w * (p - label)
        gp = ((-w * label) / (pr + eps) + (w * (f32(1) - label)) / (q + eps)).astype(f32)
    delta = (gp * q * pr).astype(f32)
    dh = (delta / f32(h)).astype(f32)
    grads = {
        "UserPreference.weight": (delta @ Pp).astype(f32),
        "PoiPreference.weight": (delta[:, None] * up[None, :]).astype(f32),
        "GeoSusceptibility.weight": (dh[:, None] * T).astype(f32),
        # dGr [D, h] laid flat IS the gradient of the [h, D] gather (the reshape is a reinterpretation)
        "GeoInfluence.weight": ((dh[:, None] * Hs).T @ F).astype(f32).reshape(-1).reshape(h, D),
    }
    return dict(pred=pr, score=s, loss=np.sum(terms, dtype=f32), terms=terms, delta=delta, grads=grads)


def dense_grads(p, user, hist, target, grads):
    """The four [rows, D] gradients torch holds after backward() (zero outside the batch's rows)."""
    out = {n: np.zeros_like(p[n], dtype=f32) for n in PARAM_NAMES}
    out["UserPreference.weight"][int(user)] = grads["UserPreference.weight"]
    t = np.asarray(target, dtype=np.int64).reshape(-1)
    hs = np.asarray(hist, dtype=np.int64).reshape(-1)
    np.add.at(out["PoiPreference.weight"], t, grads["PoiPreference.weight"])
    np.add.at(out["GeoSusceptibility.weight"], t, grads["GeoSusceptibility.weight"])
    np.add.at(out["GeoInfluence.weight"], hs, grads["GeoInfluence.weight"])
    return out


def sgd(p, g, lr, wd):
    """torch.optim.SGD without momentum: g' = g + wd * p; p -= lr * g' (fp32, every element)."""
    out = {}
    for n in PARAM_NAMES:
        gg = g[n] if wd == 0 else (g[n] + f32(wd) * p[n]).astype(f32)
        out[n] = (p[n].astype(f32) - f32(lr) * gg).astype(f32)
    return out


def step(p, a, b, user, hist, target, label, freq, dist, lr, wd):
    """One full step: (new parameters, step_grads' result with 'dense' gradients added)."""
    r = step_grads(p, a, b, user, hist, target, label, freq, dist)
    r["dense"] = dense_grads(p, user, hist, target, r["grads"])
    return sgd(p, r["dense"], lr, wd), r


def param_tolerance(g_dense_max, p_ref, lr, steps=1, grad_rtol=1e-4):
    """The per-element trajectory tolerance: steps * (lr * GRAD_RTOL * max|g| of the tensor +
    2 ulp(p_ref)) -- the gradient tolerance carried through the updates plus the two roundings of
    each update."""
    return steps * (lr * grad_rtol * float(g_dense_max) + 2.0 * np.spacing(np.abs(p_ref).astype(f32)).astype(np.float64))


_fixture = {}


def fixture():
    """tests/golden/geoie_train.npz beside the geoie.npz fixture it shares its data with."""
    if not _fixture:
        from _helpers import load_golden
        _fixture.update(z=load_golden("geoie_train.npz"), fx=go.fixture())
    return _fixture


def traj_batch(z, k):
    pre = f"step{k}/"
    return dict(user=int(z[pre + "user"][0]), hist=z[pre + "history"][0], history=z[pre + "history"],
                user_id=z[pre + "user"], target=z[pre + "target"], label=z[pre + "label"],
                freq=z[pre + "freq"], dist=z[pre + "distances"])


def saturating_case():
    """A batch known ON THE CPU to hold label-0 rows whose p rounds to exactly 1.0: the fixture's
    'sat' parameters and batch. Returns (params, a, b, batch dict, oracle result)."""
    f = fixture()
    z = f["z"]
    p = {n: z[f"sat/{n}"] for n in PARAM_NAMES}
    a, b = (float(v) for v in z["sat/ab"])
    bt = dict(user=int(z["sat/user"][0]), hist=z["sat/history"][0], history=z["sat/history"],
              user_id=z["sat/user"], target=z["sat/target"], label=z["sat/label"], freq=z["sat/freq"],
              dist=z["sat/distances"])
    r = step_grads(p, a, b, bt["user"], bt["hist"], bt["target"], bt["label"], bt["freq"], bt["dist"])
    return p, a, b, bt, r
