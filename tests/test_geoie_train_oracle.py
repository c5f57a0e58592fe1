"""tests/_geoie_train_oracle.py (the numpy restatement the GPU training tests compare with) pinned
to the reference: the gradients in tests/golden/geoie.npz and the three-step SGD trajectories and
the saturated batch in tests/golden/geoie_train.npz. No GPU."""
import numpy as np
import pytest

import _geoie_oracle as go
import _geoie_train_oracle as gt
from _helpers import GRAD_RTOL, SCORE_ATOL

TAGS = ("init", "spread")


@pytest.fixture(scope="module")
def f():
    return gt.fixture()


@pytest.mark.parametrize("tag", TAGS)
def test_gradients_match_reference(f, tag):
    z, t = f["fx"]["z"], f["fx"]["tags"][tag]
    pre = f"{tag}/train/"
    user, hist = int(z[pre + "user"][0]), z[pre + "history"][0]
    r = gt.step_grads(t["p"], t["a"], t["b"], user, hist, z[pre + "target"], z[pre + "label"],
                      z[pre + "freq"], z[pre + "distances"])
    assert np.max(np.abs(r["pred"] - z[pre + "prediction"].reshape(-1))) <= SCORE_ATOL
    assert abs(float(r["loss"]) - float(z[pre + "loss"])) <= 1e-5 * abs(float(z[pre + "loss"]))
    dense = gt.dense_grads(t["p"], user, hist, z[pre + "target"], r["grads"])
    for n in gt.PARAM_NAMES:
        ref = z[pre + "grad/" + n]
        d = np.max(np.abs(dense[n] - ref))
        print(f"{tag} {n}: max |dg| {d:.3g} of max |g| {np.max(np.abs(ref)):.3g}")
        assert d <= GRAD_RTOL * np.max(np.abs(ref)), n


@pytest.mark.parametrize("wd", (0.0, 1e-3))
@pytest.mark.parametrize("tag", TAGS)
def test_trajectory_matches_reference(f, tag, wd):
    z, t = f["z"], f["fx"]["tags"][tag]
    lr = float(z["lr"])
    p = {n: t["p"][n].copy() for n in gt.PARAM_NAMES}
    pre = f"{tag}/wd{wd:g}/"
    for k in range(gt.TRAJ_STEPS):
        bt = gt.traj_batch(z, k)
        p, r = gt.step(p, t["a"], t["b"], bt["user"], bt["hist"], bt["target"], bt["label"],
                       bt["freq"], bt["dist"], lr, wd)
        assert np.max(np.abs(r["pred"] - z[pre + f"step{k}/prediction"])) <= SCORE_ATOL
        ref = float(z[pre + f"step{k}/loss"])
        assert abs(float(r["loss"]) - ref) <= 1e-5 * abs(ref)
    worst = 0.0
    for n in gt.PARAM_NAMES:
        ref = z[pre + "final/" + n]
        tol = gt.param_tolerance(float(z[pre + "gmax/" + n]), ref, lr, gt.TRAJ_STEPS, GRAD_RTOL)
        frac = float(np.max(np.abs(p[n].astype(np.float64) - ref) / tol))
        print(f"{tag} wd={wd:g} {n}: max deviation {frac:.3g} of the trajectory tolerance")
        worst = max(worst, frac)
    # measured, as M_ULPS in _geoie_oracle.py: the oracle sits this far from the reference
    assert worst <= gt.ORACLE_DEV_FRACTION, worst
    assert gt.ORACLE_DEV_FRACTION <= 0.5   # so the GPU tests keep the plain trajectory tolerance


def test_untouched_rows_of_reference_trajectory(f):
    """weight_decay 0: the reference itself leaves every row outside the three batches bit-identical."""
    z, t = f["z"], f["fx"]["tags"]["spread"]
    tg = np.concatenate([z[f"step{k}/target"] for k in range(3)])
    keep = np.setdiff1d(np.arange(f["fx"]["P"]), tg)
    for n in ("PoiPreference.weight", "GeoSusceptibility.weight"):
        assert np.array_equal(z["spread/wd0/final/" + n][keep], t["p"][n][keep]), n


def test_fixture_holds_saturated_rows(f):
    """Label-0 rows whose prediction rounds to exactly 1.0: the reference's gradient there is
    exactly zero (the composed form), and so is the oracle's."""
    z = f["z"]
    p, a, b, bt, r = gt.saturating_case()
    sat = (z["sat/prediction"] == 1.0) & (bt["label"] == 0)
    assert sat.sum() >= 1
    assert np.array_equal((r["pred"] == 1.0) & (bt["label"] == 0), sat)
    assert np.all(z["sat/grad/PoiPreference.weight"][sat] == 0)
    assert np.all(z["sat/grad/GeoSusceptibility.weight"][sat] == 0)
    assert np.all(r["delta"][sat] == 0)
    assert np.all(r["grads"]["PoiPreference.weight"][sat] == 0)
    assert np.all(r["grads"]["GeoSusceptibility.weight"][sat] == 0)
    # w (p - label), the simplified form, would NOT be zero there
    assert np.all(go.wuj(bt["freq"].reshape(-1))[sat] * (r["pred"][sat] - bt["label"][sat]) != 0)
    for n in gt.PARAM_NAMES:
        ref = z["sat/grad/" + n]
        assert np.max(np.abs(r["grads"][n] - ref)) <= GRAD_RTOL * np.max(np.abs(ref)), n
    assert abs(float(r["loss"]) - float(z["sat/loss"])) <= 1e-5 * abs(float(z["sat/loss"]))
