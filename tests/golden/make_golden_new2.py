"""Capture the New2 fixture from the reference itself (run HERE only; never on the GPU box).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_new2.py REFERENCE_DIR
(REFERENCE_DIR = a checkout of muyeon-jo/POI_recommendation_models)

Writes tests/golden/new2.npz: P = 300 POIs, d = H = 16, R = 12 regions, U = 24 users with
histories of 2..40 POIs (one user at 2, one at 40), visit counts 1..5, 12 held-out positives per
user. Coordinates lie in data.write_synthetic's Tokyo box; POIs 5 and 17 share one coordinate
(distance 0, geo = 1) and POI 123 lies about 300 km north (geo underflows to 0 wherever lambda is
-1). The file records the coordinates and the [P, P] float32 distance matrix the model sees.

The `haversine` package is not installed here: run_new.haversine_vector is replaced by the
package's formula restated in numpy (tests/_new2_oracle.haversine_km: float64 kilometres, mean
radius 6371.0088, its operation order). Whether that equals the package bit for bit could not be
checked here; the model's parity does not depend on it, the distance block being an input.

Two parameter tags: `init` (the reference's own initialisation) and `spread` (embeddings
N(0, 0.3), embed_dist N(0, 0.5)). Per tag, from the reference's real model.New2:
  forward (model.py:959-1020) at (b, n) = (2, 2), (7, 5), (40, 13) with per-row histories, one
  target of each inside its history, a distance block of a tenth of the matrix's distances;
  the evaluation loop of run_new.py:551-570, restated line by line around the reference's own
  run_new.testDataset2 and DataLoader (the reference has no function for it): every user's score
  row, the top-50 lists and the 6-tuple of eval_metrics.evaluate_mp.
run_new.testDataset2 reads the module's global `train_matrix` (run_new.py:243); it is set here.
The script asserts that the dataset's candidates come in ascending POI id (CPython iterates the
complement set in that order here), that every captured score is within E of the float64 oracle
(tests/_new2_oracle.py), and prints the worst fraction. For `spread` it takes the next seed until
G[j] > 0 and G[j] < 0 each hold for at least a quarter of the (user, history item) pairs and no
validation or test positive lies within 2E of a k_list boundary (margins_ok, as
make_golden_new1.py).
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import Args, load_params, load_reference  # noqa: E402
import _new1_oracle as no  # noqa: E402
import _new2_oracle as n2  # noqa: E402

P, D, R, U = 300, 16, 12, 24
BETA = 0.5
K_LIST = [5, 10, 15, 20, 25, 30]
FWD = [(2, 2), (7, 5), (40, 13)]
TAGS = ("init", "spread")


def make_inputs():
    rng = np.random.default_rng(2027)
    hl = rng.integers(3, 40, U)
    hl[3], hl[9] = 2, 40
    indptr, indices, data = [0], [], []
    for h in hl:
        indices.extend(np.sort(rng.choice(P, int(h), replace=False)).tolist())
        data.extend(rng.integers(1, 6, int(h)).tolist())
        indptr.append(len(indices))
    indptr, indices = np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int64)
    data = np.array(data, dtype=np.float64)
    region_of = rng.integers(0, R, P).astype(np.int64)
    coords = np.stack([rng.uniform(35.5, 35.8, P), rng.uniform(139.5, 139.9, P)], 1)
    coords[17] = coords[5]
    coords[123] = (38.35, 139.7)
    val, test = [], []
    for u in range(U):
        comp = np.setdiff1d(np.arange(P), indices[indptr[u]:indptr[u + 1]])
        pick = rng.choice(comp, 12, replace=False)
        val.append([int(x) for x in pick[:5]])
        test.append([int(x) for x in pick[5:]])
    return indptr, indices, data, region_of, coords, val, test


def tag_params(torch, model, tag, seed):
    torch.manual_seed(seed)
    m = model.New2(P, D, D, BETA, R, U)
    p = {k: v.numpy().copy() for k, v in m.state_dict().items()}
    if tag == "spread":
        srng = np.random.default_rng(seed)
        for k in ("embed_target.weight", "embed_region.weight"):
            p[k] = (0.3 * srng.standard_normal(p[k].shape)).astype(np.float32)
        p["embed_dist"] = (0.5 * srng.standard_normal(p["embed_dist"].shape)).astype(np.float32)
    return m, p


def margins_ok(rows, E, val, test):
    """make_golden_new1.margins_ok: every positive stays inside, or outside, the first k whatever
    two evaluations within E of the exact score do."""
    for u in range(U):
        ok = ~np.isnan(rows[u])
        s, t = rows[u][ok].astype(np.float64), 2.0 * E[u][ok]
        idx = {int(c): i for i, c in enumerate(np.flatnonzero(ok))}
        for pos in val[u] + test[u]:
            i = idx[pos]
            reach = int(np.sum(s + t >= s[i] - t[i])) - 1
            above = int(np.sum(s - t > s[i] + t[i]))
            for k in K_LIST:
                if not (reach < k or above >= k):
                    return False
    return True


def evaluation_loop(torch, run_new, eval_metrics, m, dataset, val, test):
    """run_new.py:551-570 (DEVICE = cpu), keeping every prediction row."""
    from torch.utils.data import DataLoader
    rows = np.full((U, P), np.nan, dtype=np.float32)                # history POIs stay NaN
    rec = []
    with torch.no_grad():
        for user_id, (user_history, target_list, _, user_history_region, train_data_region,
                      visit_rate, dist_mat, uid) in enumerate(DataLoader(dataset, batch_size=1,
                                                                         shuffle=False)):
            user_history = user_history.squeeze(0)
            target_list = target_list.squeeze(0)
            user_history_region = user_history_region.squeeze(0)
            train_data_region = train_data_region.squeeze(0)
            visit_rate = visit_rate.squeeze(0)
            dist_mat = dist_mat.squeeze(0)
            uid = uid.squeeze(0)
            assert int(uid) == user_id and uid.dim() == 0
            t = target_list.numpy()
            assert np.all(np.diff(t) > 0), "the complement set did not iterate in ascending order"
            assert tuple(dist_mat.shape) == (user_history.shape[1], len(t))
            prediction = m(user_history, target_list, user_history_region, train_data_region,
                           visit_rate, dist_mat, uid)
            _, indices = torch.topk(prediction, Args.topk)
            rec.append([target_list[i].item() for i in indices])
            rows[user_id, t] = prediction.numpy()
    pv, rv, hv = eval_metrics.evaluate_mp(val, rec, K_LIST)
    pt, rt, ht = eval_metrics.evaluate_mp(test, rec, K_LIST)
    return rows, rec, (pv, rv, hv, pt, rt, ht)


def main(ref_path):
    import scipy.sparse as sp
    import torch
    torch.set_num_threads(4)
    model, validation, powerLaw, eval_metrics, run = load_reference(ref_path)
    import run_new                                             # imports with the same stubs

    indptr, indices, data, region_of, coords, val, test = make_inputs()
    X = sp.csr_matrix((data, indices, indptr), shape=(U, P))
    run_new.train_matrix = X                                   # the global of run_new.py:243
    run_new.haversine_vector = lambda a, b, comb=True: n2.haversine_km(a, b)
    dataset = run_new.testDataset2(X, region_of, coords)
    dist64 = dataset.POI_POI_distance.numpy()
    dist32 = dist64.astype(np.float32)
    assert dist32[5, 17] == 0.0 and 280.0 < dist32[123].max() < 330.0
    assert np.array_equal(dist32, dist32.T)
    rate = no.visit_rates(indptr, indices, data, P).astype(np.float32).astype(np.float64)
    out = dict(indptr=indptr, indices=indices, data=data, region_of=region_of, coords=coords,
               dist=dist32, num_pois=np.int64(P), num_users=np.int64(U), embed_dim=np.int64(D),
               num_regions=np.int64(R), beta=np.float64(BETA),
               k_list=np.array(K_LIST, dtype=np.int64),
               val_flat=np.array(sum(val, []), dtype=np.int64),
               val_len=np.array([len(x) for x in val], dtype=np.int64),
               test_flat=np.array(sum(test, []), dtype=np.int64),
               test_len=np.array([len(x) for x in test], dtype=np.int64))

    prng = np.random.default_rng(11)
    fwd_in = {}
    for b, n in FWD:
        hist = np.stack([prng.choice(P, n, replace=False) for _ in range(b)]).astype(np.int64)
        target = np.array([prng.choice(np.setdiff1d(np.arange(P), hist[i])) for i in range(b)],
                          dtype=np.int64)
        target[b // 2] = hist[b // 2, n - 1]                       # a target inside its history
        hreg = prng.integers(0, R, (b, n)).astype(np.int64)
        treg = prng.integers(0, R, b).astype(np.int64)
        vr = prng.uniform(0.01, 1.0, n)
        # [n, b] float64, as the dataset's; a tenth of the matrix's distances (1..4 km), so that
        # geo is of the attention weights' size and its indexing shows in the prediction
        block = 0.1 * dist64[hist[0]][:, target]
        uid = int(prng.integers(0, U))
        fwd_in[(b, n)] = (hist, target, hreg, treg, vr, block, uid)
        pre = f"fwd{b}x{n}/"
        out[pre + "history"], out[pre + "target"] = hist, target
        out[pre + "history_region"], out[pre + "target_region"], out[pre + "visit_rate"] = hreg, treg, vr
        out[pre + "dist_mat"], out[pre + "uid"] = block, np.int64(uid)

    for tag in TAGS:
        for seed in range(1000):
            m, params = tag_params(torch, model, tag, seed)
            load_params(torch, m, params)
            m.eval()
            if tag == "spread":
                pos = neg = tot = 0
                for u in range(U):
                    hist = indices[indptr[u]:indptr[u + 1]]
                    cands = np.setdiff1d(np.arange(P), hist)
                    w = params["embed_dist"][u].astype(np.float64)
                    G = w[region_of[hist]] * w[region_of[cands]].sum()
                    pos, neg, tot = pos + int((G > 0).sum()), neg + int((G < 0).sum()), tot + len(G)
                if 4 * pos < tot or 4 * neg < tot:
                    continue
            rows, rec, metrics = evaluation_loop(torch, run_new, eval_metrics, m, dataset, val, test)
            Efull = np.full((U, P), np.nan)
            worst = 0.0
            for u in range(U):
                cands, s, E = n2.user_row(params, BETA, indptr, indices, rate, region_of, dist32, u)
                assert not np.isnan(rows[u, cands]).any() and not np.isnan(s).any(), (tag, u)
                dev = np.abs(rows[u, cands].astype(np.float64) - s)
                assert np.all(dev <= E), (tag, u, float((dev / E).max()))
                worst = max(worst, float((dev / E).max()))
                Efull[u, cands] = E
            if tag == "init" or margins_ok(rows, Efull, val, test):
                break
        else:
            raise SystemExit("no seed with the margins")
        print(tag, "seed", seed, "rows: worst dev / E", worst, "max 2E", 2 * np.nanmax(Efull))
        if tag == "spread":
            print("  G > 0:", pos / tot, " G < 0:", neg / tot)
        out[f"{tag}/seed"] = np.int64(seed)
        for k, v in params.items():
            out[f"{tag}/{k}"] = v
        out[f"{tag}/rows"] = rows
        out[f"{tag}/topk_ids"] = np.array(rec, dtype=np.int64)
        out[f"{tag}/topk_scores"] = np.take_along_axis(rows, out[f"{tag}/topk_ids"], 1)
        out[f"{tag}/metrics"] = np.array(metrics, dtype=np.float64)
        if tag == "init":
            sd = m.state_dict()
            out["state_names"] = np.array(list(sd.keys()))
            out["state_shapes"] = np.array([list(v.shape) for v in sd.values()], dtype=np.int64)
        worst = 0.0
        for (b, n), (hist, target, hreg, treg, vr, block, uid) in fwd_in.items():
            with torch.no_grad():
                pred = m(torch.from_numpy(hist), torch.from_numpy(target), torch.from_numpy(hreg),
                         torch.from_numpy(treg), torch.from_numpy(vr), torch.from_numpy(block),
                         torch.tensor(uid))
            s, E = n2.score_rows(params, BETA, hist, hreg, vr.astype(np.float32), target, treg,
                                 block, uid)
            dev = np.abs(pred.numpy().astype(np.float64) - s)
            ok = ~np.isnan(s)
            assert np.array_equal(np.isnan(pred.numpy()), ~ok) and np.all(dev[ok] <= E[ok]), (tag, b, n)
            worst = max(worst, float((dev[ok] / E[ok]).max()))
            out[f"{tag}/fwd{b}x{n}/prediction"] = pred.numpy()
            if tag == "spread" and b > 2:   # both oddities must show: the "fixed" variants miss
                for variant in ("dist_transposed", "per_row_G"):
                    s2, _ = n2.score_rows(params, BETA, hist, hreg, vr.astype(np.float32), target,
                                          treg, block, uid, **{variant: True})
                    assert np.any(np.abs(pred.numpy()[ok] - s2[ok]) > 2 * E[ok]), (variant, b, n)
        print(tag, "forward: worst dev / E", worst)

    path = os.path.join(HERE, "new2.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
