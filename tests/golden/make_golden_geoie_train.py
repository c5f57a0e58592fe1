"""Capture the GeoIE training fixture from the reference itself (run HERE only; never on the GPU box).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_geoie_train.py REFERENCE_DIR
(REFERENCE_DIR = a checkout of muyeon-jo/POI_recommendation_models)

Writes tests/golden/geoie_train.npz from make_golden_geoie.make_inputs() (the data of geoie.npz)
and that fixture's two parameter sets ('init', 'spread'):
  step{k}/*   three get_GeoIE_batch batches (batches.py:204-242), users 0 (h = 1), 1 (h = 2) and 11
              (h = 45, b = 225), drawn once with a fixed seed and shared by every trajectory;
  {tag}/wd{w}/*   for weight_decay w in {0, 1e-3}: model.GeoIE + torch.optim.SGD(lr = 0.01, w)
              stepped through those batches as run.py:705-715 -- each step's loss and prediction,
              the largest |dense gradient| of every table over the steps, and the four tables
              after the third step;
  sat/*       the 'spread' parameters times 8 and the user-11 batch: predictions that round to
              exactly 1.0 on label-0 rows, with the reference's loss, prediction and gradients.
"""
from __future__ import annotations

import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import load_params, load_reference  # noqa: E402
from make_golden_geoie import D, P, U, make_inputs  # noqa: E402

LR = 0.01
DECAYS = (0.0, 1e-3)
USERS = (0, 1, 11)
SAT_SCALE = 8.0


def main(ref_path):
    import scipy.sparse as sp
    import torch
    torch.set_num_threads(4)
    model, validation, powerLaw, eval_metrics, run = load_reference(ref_path)
    import batches

    coords, indptr, indices, data, val, test = make_inputs()
    X = sp.csr_matrix((data, indices, indptr), shape=(U, P))
    dist_mat = run.distance_mat(P, [tuple(c) for c in coords.tolist()])       # run.py:40-46
    base = np.load(os.path.join(HERE, "geoie.npz"))
    out = dict(lr=np.float64(LR), decays=np.array(DECAYS), users=np.array(USERS, dtype=np.int64))

    random.seed(23)
    bts = [batches.get_GeoIE_batch(X, P, P, u, 4, dist_mat) for u in USERS]
    names = ("user", "history", "target", "label", "freq", "distances")
    for k, bt in enumerate(bts):
        for n, t in zip(names, bt):
            out[f"step{k}/{n}"] = t.numpy()

    def wd_of(opt):
        return float(opt.param_groups[0]["weight_decay"])

    def run_step(m, opt, bt):
        uidt, hist, tgt, label, freq, dist = bt
        opt.zero_grad()
        pred, w = m(uidt, tgt, hist, freq, dist)                              # run.py:708
        loss = m.loss_function(pred, label.unsqueeze(1), w)                   # run.py:710
        loss.backward()
        g = {k: v.grad.numpy().copy() for k, v in m.named_parameters()}
        gw = {k: float(np.abs(g[k] + wd_of(opt) * v.detach().numpy()).max()) for k, v in m.named_parameters()}
        opt.step()
        g["seen"] = gw
        return pred.detach().numpy().reshape(-1), np.float32(loss.item()), g

    for tag in ("init", "spread"):
        a, b = (float(v) for v in base[f"{tag}/ab"])
        for wd in DECAYS:
            m = model.GeoIE(U, P, D, 4, a, b)
            load_params(torch, m, {k: base[f"{tag}/{k}"] for k in m.state_dict()})
            m.train()
            opt = torch.optim.SGD(m.parameters(), lr=LR, weight_decay=wd)      # run.py:687
            pre = f"{tag}/wd{wd:g}/"
            gmax = {k: 0.0 for k, _ in m.named_parameters()}
            for k, bt in enumerate(bts):
                pred, loss, g = run_step(m, opt, bt)
                out[pre + f"step{k}/prediction"], out[pre + f"step{k}/loss"] = pred, loss
                for n in gmax:   # the gradient SGD sees (weight decay included)
                    gmax[n] = max(gmax[n], g["seen"][n])
            for n, v in m.state_dict().items():
                out[pre + "final/" + n] = v.numpy().copy()
                out[pre + "gmax/" + n] = np.float64(gmax[n])

    a, b = (float(v) for v in base["spread/ab"])
    m = model.GeoIE(U, P, D, 4, a, b)
    sat = {k: (SAT_SCALE * base[f"spread/{k}"]).astype(np.float32) for k in m.state_dict()}
    load_params(torch, m, sat)
    m.train()
    opt = torch.optim.SGD(m.parameters(), lr=LR)
    pred, loss, g = run_step(m, opt, bts[2])
    for n, t in zip(names, bts[2]):
        out[f"sat/{n}"] = t.numpy()
    out["sat/ab"] = np.array([a, b])
    out["sat/prediction"], out["sat/loss"] = pred, loss
    tg, hs = bts[2][2].numpy(), bts[2][1].numpy()[0]
    for n in sat:
        out[f"sat/{n}"] = sat[n]
    # the gradient rows of the batch, in batch order (every other row of the dense gradients is 0)
    out["sat/grad/UserPreference.weight"] = g["UserPreference.weight"][int(USERS[2])]
    out["sat/grad/PoiPreference.weight"] = g["PoiPreference.weight"][tg]
    out["sat/grad/GeoSusceptibility.weight"] = g["GeoSusceptibility.weight"][tg]
    out["sat/grad/GeoInfluence.weight"] = g["GeoInfluence.weight"][hs]
    lab = bts[2][3].numpy()
    print("saturated label-0 rows (p == 1.0):", int(np.sum((pred == 1.0) & (lab == 0))),
          "of", len(lab), "; non-finite loss:", not np.isfinite(loss))

    path = os.path.join(HERE, "geoie_train.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
