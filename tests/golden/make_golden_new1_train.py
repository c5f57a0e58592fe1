"""Capture the New1 training fixture from the reference itself (run HERE only; never on the GPU box).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_new1_train.py REFERENCE_DIR
(REFERENCE_DIR = a checkout of muyeon-jo/POI_recommendation_models)

Writes tests/golden/new1_train.npz from the data and parameters of new1.npz (P = 700, d = 16,
R = 16):
  step{k}/*   three batches of run_new.trainDataset.__getitem__ (run_new.py:107-137, NUM_NG
              negatives per positive) under a seeded `random`, users 4 (n = 2), 1 (n = 13) and 11
              (n = 60), drawn once and shared by every trajectory;
  watch       the embed_target rows the fixture records: every row one of the three batches
              touches plus N_UNTOUCHED rows none of them touches (embed_target's gradient is
              asserted zero outside the rows of its own batch);
  {tag}/wd{w}/step{k}/*   for tag in ('init', 'spread') and weight_decay w in {0, 1e-7, 1e-3}:
              model.New1 + loss_func + backward + torch.optim.Adam(lr = 0.01, weight_decay = w)
              stepped through those batches as run_new.py:403-410 -- per step the prediction, the
              loss, the five gradients and the parameters, exp_avg and exp_avg_sq afterwards
              (embed_target's at the watch rows, the other four tensors whole);
  sat/*       one trainDataset batch on the 'spread' parameters with attn_V scaled (searched over
              scale, user and seed) that holds a label-0 row with x == 1.0f, a label-1 row with
              x (1 - x) < 1e-12 and x > 0, and a label-1 row with x == 0 (asserted): prediction,
              loss, delta = d loss / d (the sigmoid's input) and the five gradients;
  n1/*        the record that the reference raises at n = 1 (inside BCELoss).
The script asserts that the float64 oracle (tests/_new1_train_oracle.py) reproduces every recorded
prediction, loss and gradient within the tolerances of tests/test_new1_train_oracle.py.
"""
from __future__ import annotations

import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import load_params, load_reference  # noqa: E402
import _new1_train_oracle as to  # noqa: E402

LR = 0.01
DECAYS = (0.0, 1e-7, 1e-3)
USERS = (4, 1, 11)
NUM_NG = 2
N_UNTOUCHED = 8
NAMES = to.NAMES


def main(ref_path):
    import scipy.sparse as sp
    import torch
    torch.set_num_threads(4)
    model, validation, powerLaw, eval_metrics, run = load_reference(ref_path)
    import run_new

    base = np.load(os.path.join(HERE, "new1.npz"))
    P, U, D, R = (int(base[k]) for k in ("num_pois", "num_users", "embed_dim", "num_regions"))
    beta = float(base["beta"])
    X = sp.csr_matrix((base["data"], base["indices"], base["indptr"]), shape=(U, P))
    region_of = base["region_of"]
    hl = np.diff(base["indptr"])
    assert [int(hl[u]) for u in USERS] == [2, 13, 60]
    ds = run_new.trainDataset(X, region_of, NUM_NG)
    out = dict(lr=np.float64(LR), decays=np.array(DECAYS), users=np.array(USERS, dtype=np.int64),
               num_ng=np.int64(NUM_NG))
    names = ("history", "target", "label", "history_region", "target_region", "visit_rate")

    random.seed(29)
    bts = [ds[u] for u in USERS]
    touched = np.zeros(P, bool)
    for k, bt in enumerate(bts):
        for nm, t in zip(names, bt):
            out[f"step{k}/{nm}"] = t.numpy()[0] if nm.startswith("history") else t.numpy()
        touched[bt[1].numpy()] = True
        touched[bt[0].numpy()[0]] = True
    free = np.flatnonzero(~touched)
    watch = np.sort(np.concatenate([np.flatnonzero(touched), free[:: len(free) // N_UNTOUCHED][:N_UNTOUCHED]]))
    out["watch"] = watch

    def run_step(m, opt, bt, hook_delta=False):
        hist, tgt, label, hreg, treg, vr = bt
        opt.zero_grad()
        keep = []
        hk = None
        if hook_delta:
            def grab(mod, inp):
                inp[0].retain_grad()
                keep.append(inp[0])
            hk = m.sigmoid.register_forward_pre_hook(grab)
        pred = m(hist, tgt, hreg, treg, vr)                       # run_new.py:406
        if hk is not None:
            hk.remove()
        loss = m.loss_func(pred, label)                           # run_new.py:407
        loss.backward()
        g = {k: v.grad.numpy().copy() for k, v in m.named_parameters()}
        opt.step()
        delta = keep[0].grad.numpy().copy() if keep else None
        return pred.detach().numpy().reshape(-1), np.float32(loss.item()), g, delta

    def check_oracle(params, bt, pred, loss, g):
        hist, tgt, label, hreg, treg, vr = (t.numpy() for t in bt)
        x, lo, dl, og = to.step_grads(params, beta, hist[0], tgt, label, hreg[0], treg,
                                      vr.astype(np.float32))
        assert np.all(np.abs(x - pred) <= 1e-4), float(np.abs(x - pred).max())
        assert abs(lo - float(loss)) <= 1e-5 * abs(float(loss)), (lo, float(loss))
        for k in NAMES:
            lim = 1e-4 * np.abs(g[k]).max()
            assert np.all(np.abs(og[k] - g[k]) <= lim), (k, float(np.abs(og[k] - g[k]).max()), lim)
        return dl

    for tag in ("init", "spread"):
        for wd in DECAYS:
            m = model.New1(P, D, D, beta, R)
            load_params(torch, m, {k: base[f"{tag}/{k}"] for k in NAMES})
            m.train()
            opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=wd)   # run_new.py:389
            for k, bt in enumerate(bts):
                before = {n: v.detach().numpy().copy() for n, v in m.named_parameters()}
                pred, loss, g, _ = run_step(m, opt, bt)
                check_oracle(before, bt, pred, loss, g)
                pre = f"{tag}/wd{wd:g}/step{k}/"
                out[pre + "prediction"], out[pre + "loss"] = pred, loss
                mask = np.ones(P, bool)
                mask[watch] = False
                assert not g[NAMES[0]][mask].any()
                for n, v in m.named_parameters():
                    st = opt.state[v]
                    assert int(st["step"]) == k + 1
                    sel = (lambda a: a[watch]) if n == NAMES[0] else (lambda a: a)
                    out[pre + "grad/" + n] = sel(g[n])
                    out[pre + "param/" + n] = sel(v.detach().numpy().copy())
                    out[pre + "exp_avg/" + n] = sel(st["exp_avg"].numpy().copy())
                    out[pre + "exp_avg_sq/" + n] = sel(st["exp_avg_sq"].numpy().copy())

    # the saturated batch: attn_V of 'spread' scaled until one batch holds all three kinds of row
    found = None
    for scale in (200.0, 400.0, 800.0, 1600.0, 100.0):
        sat = {k: base[f"spread/{k}"].copy() for k in NAMES}
        sat["attn_V.weight"] = (sat["attn_V.weight"] * np.float32(scale)).astype(np.float32)
        m = model.New1(P, D, D, beta, R)
        load_params(torch, m, sat)
        m.train()
        for u in range(U):
            if hl[u] < 2:
                continue
            random.seed(1000 + u)
            bt = ds[u]
            with torch.no_grad():
                x = m(*[bt[i] for i in (0, 1, 3, 4, 5)]).numpy()
            lab = bt[2].numpy()
            with np.errstate(all="ignore"):
                xx = x.astype(np.float32) * (np.float32(1) - x.astype(np.float32))
            c0 = (lab == 0) & (x == 1.0)
            c1 = (lab == 1) & (xx < 1e-12) & (x > 0)
            c2 = (lab == 1) & (x == 0)
            if c0.any() and c1.any() and c2.any() and not np.isnan(x).any():
                found = (scale, u, bt, sat)
                break
        if found:
            break
    assert found, "no saturated batch found"
    scale, u, bt, sat = found
    m = model.New1(P, D, D, beta, R)
    load_params(torch, m, sat)
    m.train()
    opt = torch.optim.Adam(m.parameters(), lr=LR)
    pred, loss, g, delta = run_step(m, opt, bt, hook_delta=True)
    lab = bt[2].numpy()
    with np.errstate(all="ignore"):
        xx = pred * (np.float32(1) - pred)
    rows0 = np.flatnonzero((lab == 0) & (pred == 1.0))
    rows1 = np.flatnonzero((lab == 1) & (xx < 1e-12) & (pred > 0))
    rows2 = np.flatnonzero((lab == 1) & (pred == 0))
    assert len(rows0) and len(rows1) and len(rows2)
    assert not delta[rows0].any() and not delta[rows2].any()
    # |delta| = x (1 - x) / 1e-12 / b on the tiny rows (0 where x is subnormal), never 1 / b
    assert np.all(np.abs(delta[rows1]) < 1.0 / len(lab)) and delta[rows1].any()
    dl = check_oracle(sat, bt, pred, loss, g)
    print("saturated: scale", scale, "user", u, "rows", len(rows0), len(rows1), len(rows2),
          "oracle delta == reference's on them:",
          bool(np.array_equal(dl[rows0], delta[rows0]) and np.array_equal(dl[rows2], delta[rows2])))
    for nm, t in zip(names, bt):
        out[f"sat/{nm}"] = t.numpy()[0] if nm.startswith("history") else t.numpy()
    out["sat/attn_V_scale"], out["sat/user"] = np.float64(scale), np.int64(u)
    out["sat/prediction"], out["sat/loss"], out["sat/delta"] = pred, loss, delta.reshape(-1)
    out["sat/rows_x1_label0"], out["sat/rows_tiny_label1"], out["sat/rows_x0_label1"] = rows0, rows1, rows2
    sat_rows = np.unique(np.concatenate([bt[0].numpy()[0], bt[1].numpy()]))
    out["sat/rows"] = sat_rows
    for n in NAMES:
        out["sat/grad/" + n] = g[n][sat_rows] if n == NAMES[0] else g[n]
    mask = np.ones(P, bool)
    mask[sat_rows] = False
    assert not g[NAMES[0]][mask].any()

    # n = 1: the reference raises inside BCELoss (its positive row has no unmasked history item)
    X1 = sp.csr_matrix((np.array([2.0, 1.0, 3.0]), np.array([5, 5, 9]), np.array([0, 1, 3])), shape=(2, P))
    ds1 = run_new.trainDataset(X1, region_of, NUM_NG)
    random.seed(3)
    bt = ds1[0]
    m = model.New1(P, D, D, beta, R)
    load_params(torch, m, {k: base[f"init/{k}"] for k in NAMES})
    try:
        m.loss_func(m(*[bt[i] for i in (0, 1, 3, 4, 5)]), bt[2])
        raised, msg = False, ""
    except RuntimeError as e:
        raised, msg = True, str(e)
    assert raised and "between 0 and 1" in msg, msg
    out["n1/raised"], out["n1/message"] = np.bool_(raised), np.str_(msg[:120])

    path = os.path.join(HERE, "new1_train.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; watch rows", len(watch))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
