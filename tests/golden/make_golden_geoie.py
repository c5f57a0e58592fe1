"""Capture the GeoIE fixture from the reference itself (run HERE only; never on the GPU box).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_geoie.py REFERENCE_DIR
(REFERENCE_DIR = a checkout of muyeon-jo/POI_recommendation_models)

Writes tests/golden/geoie.npz: seeded coordinates (two identical POIs, a pair a few metres apart
and one POI more than 100 km away, so both clamps of run.py:44 are hit), CSR histories, two
parameter sets with their power laws, and what the reference computes from them:
  model.GeoIE.forward (model.py:785-813) on get_GeoIE_batch_test batches (batches.py:244-269),
  validation.GeoIE_validation (validation.py:183-195): score rows, recommended lists, the 6-tuple,
  one get_GeoIE_batch training batch (batches.py:204-242): prediction, loss_function, gradients.
The P x P dist_mat (run.distance_mat, run.py:40-46) is NOT stored: tests rebuild it from the
coordinates with oracle.powerlaw_oracle.dist and the clamp.
"""
from __future__ import annotations

import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import Args, load_params, load_reference  # noqa: E402

P, D, U = 300, 16, 12
HIST_LEN = [1, 2, 16, 5, 7, 23, 37, 3, 11, 29, 16, 45]     # 1, 2, D, and neither divisors nor multiples
K_LIST = [5, 10, 15, 20, 25, 30]


def make_inputs():
    rng = np.random.default_rng(2024)
    coords = np.stack([35.5 + 0.3 * rng.random(P), 139.4 + 0.4 * rng.random(P)], 1)
    coords[1] = coords[0]                              # identical: dist == 0.0 -> 0.01
    coords[3] = coords[2] + np.array([5e-5, 0.0])      # ~5.6 m apart: below the 0.01 km clamp
    coords[4] = coords[4] + np.array([2.0, 0.0])       # ~220 km from the rest: above the 100 km clamp
    indptr, indices, data = [0], [], []
    for u, h in enumerate(HIST_LEN):
        hist = set(rng.choice(P, h, replace=False).tolist())
        if h >= 5:                                     # the clamp POIs sit in several histories
            hist = set(list(hist)[:h - 3]) | {0, 2, 4} if u % 2 else set(list(hist)[:h - 2]) | {1, 3}
            while len(hist) < h:
                hist.add(int(rng.integers(5, P)))
        hist = np.sort(np.array(sorted(hist), dtype=np.int64))
        assert len(hist) == h
        indices.extend(hist.tolist())
        data.extend(rng.integers(1, 6, h).tolist())
        indptr.append(len(indices))
    indptr, indices = np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int64)
    val, test = [], []
    for u in range(U):
        comp = np.setdiff1d(np.arange(P), indices[indptr[u]:indptr[u + 1]])
        pick = rng.choice(comp, 12, replace=False)
        val.append([int(x) for x in pick[:5]])
        test.append([int(x) for x in pick[5:]])
    return coords, indptr, indices, np.array(data, dtype=np.float64), val, test


def main(ref_path):
    import scipy.sparse as sp
    import torch
    torch.set_num_threads(4)
    model, validation, powerLaw, eval_metrics, run = load_reference(ref_path)
    import batches

    coords, indptr, indices, data, val, test = make_inputs()
    X = sp.csr_matrix((data, indices, indptr), shape=(U, P))
    coo = [tuple(c) for c in coords.tolist()]
    dist_mat = run.distance_mat(P, coo)                               # run.py:40-46, reference code

    np.random.seed(0)
    Gf = powerLaw.PowerLaw()
    Gf.fit_distance_distribution(X, coords)
    out = dict(coords=coords, indptr=indptr, indices=indices, data=data, num_pois=np.int64(P),
               num_users=np.int64(U), embed_dim=np.int64(D), k_list=np.array(K_LIST, dtype=np.int64),
               val_flat=np.array(sum(val, []), dtype=np.int64),
               val_len=np.array([len(x) for x in val], dtype=np.int64),
               test_flat=np.array(sum(test, []), dtype=np.int64),
               test_len=np.array([len(x) for x in test], dtype=np.int64))

    prng = np.random.default_rng(7)
    for tag, ab in (("init", (float(Gf.a), float(Gf.b))), ("spread", (0.8, -0.9))):
        torch.manual_seed(5)
        m = model.GeoIE(U, P, D, 4, ab[0], ab[1])                      # the reference's Xavier init
        if tag == "spread":
            p = {k: (0.3 * prng.standard_normal(tuple(v.shape))).astype(np.float32)
                 for k, v in m.state_dict().items()}
            load_params(torch, m, p)
        for k, v in m.state_dict().items():
            out[f"{tag}/{k}"] = v.numpy().copy()
        out[f"{tag}/ab"] = np.array(ab, dtype=np.float64)
        m.eval()

        # forward batches, built as get_GeoIE_batch_test builds them (n rows of one user's batch)
        for n, uid in ((1, 0), (7, 4), (33, 6)):
            uidt, hist, tgt, _, freq, dist = batches.get_GeoIE_batch_test(X, uid, dist_mat)
            sel = np.sort(prng.choice(len(tgt), n, replace=False))
            args = [t[sel] for t in (uidt, tgt, hist, freq, dist)]
            with torch.no_grad():
                pred, w = m(*args)
            pre = f"{tag}/fwd{n}/"
            out[pre + "user"], out[pre + "target"] = args[0].numpy(), args[1].numpy()
            out[pre + "history"], out[pre + "freq"] = args[2].numpy(), args[3].numpy()
            out[pre + "distances"] = args[4].numpy()
            out[pre + "prediction"], out[pre + "wuj"] = pred.numpy(), w.numpy()

        # the full validation: score rows through a forward hook, lists through evaluate_mp
        rows = np.full((U, P), -1.0, dtype=np.float32)
        hook = m.register_forward_hook(lambda mod, inp, o: rows.__setitem__(
            (int(inp[0][0]), inp[1].numpy()), o[0].detach().numpy().reshape(-1)))
        recs = {}
        orig = validation.eval_metrics.evaluate_mp

        def spy(positive, rec, k_list):
            recs.setdefault("rec", [list(map(int, r)) for r in rec])
            return orig(positive, rec, k_list)

        validation.eval_metrics.evaluate_mp = spy
        try:
            with torch.no_grad():
                metrics = validation.GeoIE_validation(m, Args(), U, test, val, X, K_LIST, dist_mat)
        finally:
            validation.eval_metrics.evaluate_mp = orig
            hook.remove()
        out[f"{tag}/rows"] = rows
        out[f"{tag}/topk_ids"] = np.array(recs["rec"], dtype=np.int64)
        out[f"{tag}/topk_scores"] = np.take_along_axis(rows, out[f"{tag}/topk_ids"], 1)
        out[f"{tag}/metrics"] = np.array(metrics, dtype=np.float64)

        # one training batch as get_GeoIE_batch lays it out: positives + 4 negatives each
        random.seed(11)
        uidt, hist, tgt, label, freq, dist = batches.get_GeoIE_batch(X, P, P, 3, 4, dist_mat)
        m.train()
        m.zero_grad()
        pred, w = m(uidt, tgt, hist, freq, dist)
        loss = m.loss_function(pred, label.unsqueeze(1), w)            # run.py:710
        loss.backward()
        pre = f"{tag}/train/"
        out[pre + "user"], out[pre + "target"], out[pre + "history"] = uidt.numpy(), tgt.numpy(), hist.numpy()
        out[pre + "label"], out[pre + "freq"], out[pre + "distances"] = label.numpy(), freq.numpy(), dist.numpy()
        out[pre + "prediction"], out[pre + "wuj"] = pred.detach().numpy(), w.numpy()
        out[pre + "loss"] = np.float32(loss.item())
        for k, v in m.named_parameters():
            out[pre + "grad/" + k] = v.grad.numpy().copy()

    path = os.path.join(HERE, "geoie.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; fitted (a, b) =", Gf.a, Gf.b)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
