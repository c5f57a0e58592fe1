"""The float64 oracle of the New1 training step (tests/_new1_train_oracle.py) pinned to the
reference's own steps (tests/golden/new1_train.npz), the Adam bound it derives held against the
reference's recorded fp32 updates, and trainer.New1Trainer off the device. CPU only."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _new1_train_common as tc
import _new1_train_oracle as to
from _helpers import GRAD_RTOL, SCORE_ATOL
from _new1_common import golden_params, make_model

NAMES = to.NAMES
TRAJ = [(tag, wd) for tag in tc.TAGS for wd in tc.DECAYS]


@pytest.fixture(scope="module")
def fx():
    return tc.fixtures()


def _assert_step(params, beta, batch, pred, loss, grads):
    x, lo, dl, g = to.step_grads(params, beta, *batch)
    assert np.all(np.abs(x - pred) <= SCORE_ATOL), float(np.abs(x - pred).max())
    assert abs(lo - loss) <= 1e-5 * abs(loss), (lo, loss)
    for n in NAMES:
        lim = GRAD_RTOL * np.abs(grads[n]).max()
        dev = np.abs(g[n] - grads[n]).max()
        assert dev <= lim, (n, float(dev), float(lim))
    return dl


@pytest.mark.parametrize("tag,wd", TRAJ)
def test_oracle_reproduces_the_reference_steps(fx, tag, wd):
    z, zt = fx
    beta = float(z["beta"])
    for k in range(tc.STEPS):
        params, _, _ = tc.state_before(z, zt, tag, wd, k)
        rec = tc.recorded(zt, tag, wd, k)
        _assert_step(params, beta, tc.batch_of(zt, f"step{k}/"), rec["prediction"], rec["loss"],
                     tc.full_grads(z, zt, rec, tag))


def _sat_params(z, zt):
    p = golden_params(z, "spread")
    p["attn_V.weight"] = (p["attn_V.weight"] * np.float32(float(zt["sat/attn_V_scale"]))).astype(np.float32)
    return p


def test_saturated_rows_keep_the_composed_delta(fx):
    """BCELoss after Sigmoid in autograd's composed form, pinned by the reference's own delta: 0 on
    the label-0 rows with x == 1.0f and on the label-1 rows with x == 0, x (1 - x) / 1e-12 / b on
    the label-1 rows with x (1 - x) < 1e-12 (never -1 / b ... -0.5 / b)."""
    z, zt = fx
    batch = tc.batch_of(zt, "sat/")
    b = len(batch[1])
    pred, delta = zt["sat/prediction"], zt["sat/delta"]
    r0, r1, r2 = zt["sat/rows_x1_label0"], zt["sat/rows_tiny_label1"], zt["sat/rows_x0_label1"]
    assert len(r0) and len(r1) and len(r2)
    assert np.all(pred[r0] == 1.0) and np.all(batch[2][r0] == 0)
    assert np.all(pred[r2] == 0.0) and np.all(batch[2][r2] == 1)
    # the composed form on the reference's own float32 predictions gives the reference's delta
    mine = to.delta32(pred, batch[2], b)
    assert not mine[r0].any() and not mine[r2].any() and not delta[r0].any() and not delta[r2].any()
    big = np.abs(delta) > 1e-30          # above the subnormal products
    assert np.all(np.abs(mine[big] - delta[big]) <= 4 * np.spacing(np.abs(delta[big])))
    assert np.all(np.abs(mine[r1]) < 1.0 / b) and mine[r1].any()
    # and the oracle's whole step on that batch
    grads = {n: np.zeros_like(z[f"spread/{n}"]) for n in NAMES}
    for n in NAMES:
        if n == NAMES[0]:
            grads[n][zt["sat/rows"]] = zt["sat/grad/" + n]
        else:
            grads[n] = zt["sat/grad/" + n]
    dl = _assert_step(_sat_params(z, zt), float(z["beta"]), batch, pred, float(zt["sat/loss"]), grads)
    assert not dl[r0].any() and not dl[r2].any()


def test_reference_raises_at_n1(fx):
    _, zt = fx
    assert bool(zt["n1/raised"]) and "between 0 and 1" in str(zt["n1/message"])


def test_adam_bound_holds_for_the_reference_steps(fx):
    """The oracle's Adam fed the reference's recorded gradients reproduces the reference's recorded
    parameters, exp_avg and exp_avg_sq inside the derived fp32 bound, for every element the
    fixture records, at every step of every trajectory."""
    z, zt = fx
    lr = float(zt["lr"])
    worst = 0.0
    for tag, wd in TRAJ:
        for k in range(tc.STEPS):
            params, m, v = tc.state_before(z, zt, tag, wd, k)
            rec = tc.recorded(zt, tag, wd, k)
            out, bnd = to.adam_all(params, m, v, tc.full_grads(z, zt, rec, tag), k + 1, lr, wd)
            for n in NAMES:
                for i, key in enumerate(("param", "exp_avg", "exp_avg_sq")):
                    want = rec[key][n].astype(np.float64)
                    dev = np.abs(tc.sel(zt, n, out[n][i]) - want)
                    lim = tc.sel(zt, n, bnd[n][i])
                    assert np.all(dev <= lim), (tag, wd, k, n, key, float((dev / lim).max()))
                    worst = max(worst, float((dev / lim).max()))
    print("largest deviation / bound:", worst)
    assert worst <= to.ORACLE_DEV_FRACTION, worst


def test_adam_moves_a_row_with_zero_gradient_through_exp_avg():
    """The momentum trap in the oracle itself: after one step with a gradient, a second step with
    a zero gradient and no weight decay still moves the element."""
    p, m, v = np.float32([0.5]), np.float32([0.0]), np.float32([0.0])
    (p1, m1, v1), _ = to.adam(p, m, v, np.float32([0.2]), 1, 0.01, 0.0)
    (p2, _, _), _ = to.adam(p1.astype(np.float32), m1.astype(np.float32), v1.astype(np.float32),
                            np.float32([0.0]), 2, 0.01, 0.0)
    assert p2[0] < p1[0] < 0.5


def test_trainer_off_the_device(fx):
    from poi_recommendation_models_amd import _capi, trainer
    from poi_recommendation_models_amd.model import BPR
    from _new1_common import golden_csr
    z, _ = fx
    assert _capi.ABI_VERSION == 23
    for name in ("nais_new1_make_train_batch", "nais_new1_train_step_workspace_size",
                 "nais_new1_train_step"):
        assert name in _capi.EXPORTS
    assert [f for f, _ in _capi.NaisNew1AdamState._fields_][:4] == [
        "m_embed_target", "v_embed_target", "m_embed_region", "v_embed_region"]
    assert len(_capi.NaisNew1AdamState._fields_) == 10 and len(_capi.NaisNew1TrainGrads._fields_) == 5
    X = golden_csr(z)
    m = make_model(golden_params(z, "init"), float(z["beta"]))
    with pytest.raises(RuntimeError):
        trainer.New1Trainer(m, X, z["region_of"])
    with pytest.raises(NotImplementedError):
        trainer.New1Trainer(BPR(4, 5, 2), X, z["region_of"])
    assert torch.is_grad_enabled()
