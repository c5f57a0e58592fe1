"""Shared by the New1 training tests: access to tests/golden/new1_train.npz.

The fixture records embed_target (its gradient, and its value, exp_avg and exp_avg_sq after each
step) at the `watch` rows only: every row one of the three batches touches plus a few that none
touches. `state_before` rebuilds the full tensors a step starts from: the trajectory's initial
parameters (new1.npz) and zero state, with the watch rows replaced by what the reference recorded
after the previous step. The other rows are touched by no batch, so they do not enter any forward
pass; they only have to be the same on both sides of a comparison.
"""
from __future__ import annotations

import numpy as np

import _new1_train_oracle as to
from _helpers import load_golden

NAMES = to.NAMES
TAGS = ("init", "spread")
DECAYS = (0.0, 1e-7, 1e-3)
STEPS = 3
BATCH_KEYS = ("history", "target", "label", "history_region", "target_region", "visit_rate")


def fixtures():
    return load_golden("new1.npz"), load_golden("new1_train.npz")


def batch_of(zt, pre):
    """(hist, target, labels, hreg, treg, visit rate as float32) of `pre` = 'step0/' .. or 'sat/'."""
    h, t, y, hr, tr, vr = (zt[pre + k] for k in BATCH_KEYS)
    return h, t, y, hr, tr, vr.astype(np.float32)


def widen(zt, name, a, fill):
    """The recorded array of parameter `name` as a full tensor: embed_target's watch rows over
    `fill` (a copy), any other tensor as recorded."""
    if name != NAMES[0]:
        return np.array(a, dtype=np.float32)
    out = np.array(fill, dtype=np.float32)
    out[zt["watch"]] = a
    return out


def state_before(z, zt, tag, wd, k):
    """(params, exp_avg, exp_avg_sq), full float32 tensors, before step k of trajectory (tag, wd)."""
    init = {n: np.array(z[f"{tag}/{n}"], dtype=np.float32) for n in NAMES}
    zero = {n: np.zeros_like(init[n]) for n in NAMES}
    if k == 0:
        return init, zero, {n: v.copy() for n, v in zero.items()}
    pre = f"{tag}/wd{wd:g}/step{k - 1}/"
    return ({n: widen(zt, n, zt[pre + "param/" + n], init[n]) for n in NAMES},
            {n: widen(zt, n, zt[pre + "exp_avg/" + n], zero[n]) for n in NAMES},
            {n: widen(zt, n, zt[pre + "exp_avg_sq/" + n], zero[n]) for n in NAMES})


def recorded(zt, tag, wd, k):
    """The reference's step k: dict with prediction, loss, grads (full tensors, zero outside the
    watch rows) and param / exp_avg / exp_avg_sq (as recorded: embed_target at the watch rows)."""
    pre = f"{tag}/wd{wd:g}/step{k}/"
    out = {"prediction": zt[pre + "prediction"], "loss": float(zt[pre + "loss"])}
    for key in ("grad", "param", "exp_avg", "exp_avg_sq"):
        out[key] = {n: zt[pre + f"{key}/{n}"] for n in NAMES}
    return out


def full_grads(z, zt, rec, tag):
    return {n: widen(zt, n, rec["grad"][n], np.zeros_like(z[f"{tag}/{n}"])) for n in NAMES}


def sel(zt, name, a):
    """The rows of a full tensor that the fixture records."""
    return np.asarray(a)[zt["watch"]] if name == NAMES[0] else np.asarray(a)
