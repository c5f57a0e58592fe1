"""Capture the New1 fixture from the reference itself (run HERE only; never on the GPU box).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_new1.py REFERENCE_DIR
(REFERENCE_DIR = a checkout of muyeon-jo/POI_recommendation_models)

Writes tests/golden/new1.npz: P = 700 POIs, d = H = 16, R = 16 regions, U = 40 users with
histories of 2..60 POIs (one user at 2, one at 60), visit counts 1..5, 12 held-out positives per
user, and three parameter tags -- `init` (the reference's own initialisation), `spread`
(embeddings N(0, 0.3)) and `sharp` (`spread` with attn_Q / attn_K scaled until max |a| is within
5..20 and attn_V scaled until the largest |pred| is 6, so that fewer than 1 % of the scores
saturate; both asserted). Per tag, from
the reference itself:
  model.New1.forward (model.py:861-918) at (b, n) = (2, 2), (7, 5), (40, 13), one row of each with
  its target inside its history,
  validation.New1_validation (validation.py:212-230): every user's candidate score row and visit
  rates (through a forward hook), the recommended top-50 lists, the 6-tuple.
And an `overflow` case: three rows (n = 2) on scaled parameters with every a_j at least 1 beyond
the fp32 exp's range on either side (rows 0 and 1: the reference's NaNs) or well inside it (row 2).

The script asserts that every captured score is within E of the float64 oracle
(tests/_new1_oracle.py). For `spread` and `sharp` it takes the next seed until no validation or
test positive of any user lies within 2E of a k_list boundary (margins_ok: with every score moved
by up to 2 E(u, c), each positive stays inside, or stays outside, the first k), so the 6-tuple is
the only admissible one.
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

P, D, R, U = 700, 16, 16, 40
BETA = 0.5
K_LIST = [5, 10, 15, 20, 25, 30]
FWD = [(2, 2), (7, 5), (40, 13)]


def make_inputs():
    rng = np.random.default_rng(2026)
    hl = rng.integers(3, 60, U)
    hl[4], hl[11] = 2, 60
    indptr, indices, data = [0], [], []
    for h in hl:
        indices.extend(np.sort(rng.choice(P, int(h), replace=False)).tolist())
        data.extend(rng.integers(1, 6, int(h)).tolist())
        indptr.append(len(indices))
    indptr, indices = np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int64)
    data = np.array(data, dtype=np.float64)
    region_of = rng.integers(0, R, P).astype(np.int64)
    val, test = [], []
    for u in range(U):
        comp = np.setdiff1d(np.arange(P), indices[indptr[u]:indptr[u + 1]])
        pick = rng.choice(comp, 12, replace=False)
        val.append([int(x) for x in pick[:5]])
        test.append([int(x) for x in pick[5:]])
    return indptr, indices, data, region_of, val, test


def tag_params(torch, model, tag, seed):
    torch.manual_seed(seed)
    m = model.New1(P, D, D, BETA, R)
    p = {k: v.numpy().copy() for k, v in m.state_dict().items()}
    if tag in ("spread", "sharp"):
        srng = np.random.default_rng(seed)
        for k in ("embed_target.weight", "embed_region.weight"):
            p[k] = (0.3 * srng.standard_normal(p[k].shape)).astype(np.float32)
    return m, p


def sharpen(p, indptr, indices, rate, region_of):
    """attn_Q / attn_K scaled to max |a| = 10 (asserted within 5..20); attn_V scaled until the
    largest |pred| is 6, far from the |pred| > 17 at which an fp32 sigmoid saturates."""
    def hist_of(u):
        return indices[indptr[u]:indptr[u + 1]]

    def max_logit(q):
        return max(np.abs(no.logits(q, hist_of(u), region_of[hist_of(u)], np.arange(P),
                                    region_of)).max() for u in range(U))

    def max_pred(q):
        big = 0.0
        for u in range(U):
            _, sc, _ = no.user_row(q, BETA, indptr, indices, rate, region_of, u, with_E=False)
            big = max(big, float(np.abs(np.log(sc / (1.0 - sc))).max()))
        return big

    p = dict(p)
    s = np.float32(np.sqrt(10.0 / max_logit(p)))
    p["attn_Q.weight"] = (p["attn_Q.weight"] * s).astype(np.float32)
    p["attn_K.weight"] = (p["attn_K.weight"] * s).astype(np.float32)
    amax = max_logit(p)
    assert 5.0 <= amax <= 20.0, amax
    for _ in range(3):   # the visit-rate term does not scale with attn_V: a few rounds
        p["attn_V.weight"] = (p["attn_V.weight"] * np.float32(6.0 / max_pred(p))).astype(np.float32)
    return p, amax


def margins_ok(rows, E, val, test):
    """Every positive is inside or outside the first k of its user whatever two evaluations within
    E of the exact score (so within 2E of the reference's) do: fewer than k others can reach it,
    or at least k others stay above it."""
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


def main(ref_path):
    import scipy.sparse as sp
    import torch
    torch.set_num_threads(4)
    model, validation, powerLaw, eval_metrics, run = load_reference(ref_path)

    indptr, indices, data, region_of, val, test = make_inputs()
    X = sp.csr_matrix((data, indices, indptr), shape=(U, P))
    rate = no.visit_rates(indptr, indices, data, P).astype(np.float32).astype(np.float64)
    out = dict(indptr=indptr, indices=indices, data=data, region_of=region_of,
               num_pois=np.int64(P), num_users=np.int64(U), embed_dim=np.int64(D),
               num_regions=np.int64(R), beta=np.float64(BETA),
               k_list=np.array(K_LIST, dtype=np.int64),
               val_flat=np.array(sum(val, []), dtype=np.int64),
               val_len=np.array([len(x) for x in val], dtype=np.int64),
               test_flat=np.array(sum(test, []), dtype=np.int64),
               test_len=np.array([len(x) for x in test], dtype=np.int64))

    prng = np.random.default_rng(7)
    fwd_in = {}
    for b, n in FWD:
        hist = np.stack([prng.choice(P, n, replace=False) for _ in range(b)]).astype(np.int64)
        target = prng.integers(0, P, b).astype(np.int64)
        target[b // 2] = hist[b // 2, n - 1]                       # a target inside its history
        assert all(target[i] not in hist[i] for i in range(b) if i != b // 2)
        hreg = prng.integers(0, R, (b, n)).astype(np.int64)
        treg = prng.integers(0, R, b).astype(np.int64)
        vr = prng.uniform(0.01, 1.0, n)
        fwd_in[(b, n)] = (hist, target, hreg, treg, vr)
        pre = f"fwd{b}x{n}/"
        out[pre + "history"], out[pre + "target"] = hist, target
        out[pre + "history_region"], out[pre + "target_region"], out[pre + "visit_rate"] = hreg, treg, vr

    for tag in ("init", "spread", "sharp"):
        for seed in range(1000):
            m, params = tag_params(torch, model, tag, seed)
            amax = None
            if tag == "sharp":
                params, amax = sharpen(params, indptr, indices, rate, region_of)
            load_params(torch, m, params)
            m.eval()
            rows = np.full((U, P), np.nan, dtype=np.float32)        # history POIs stay NaN
            seen_rates, count = [], [0]

            def hook(mod, inp, o):
                rows[count[0], inp[1].numpy()] = o.detach().numpy().reshape(-1)
                seen_rates.append(inp[4].numpy().astype(np.float64).copy())
                count[0] += 1

            hk = m.register_forward_hook(hook)
            recs = {}
            orig = validation.eval_metrics.evaluate_mp

            def spy(positive, rec, k_list):
                recs.setdefault("rec", [list(map(int, r)) for r in rec])
                return orig(positive, rec, k_list)

            validation.eval_metrics.evaluate_mp = spy
            try:
                metrics = validation.New1_validation(m, Args(), U, test, val, X, region_of, K_LIST)
            finally:
                validation.eval_metrics.evaluate_mp = orig
                hk.remove()
            # every captured score within E of the oracle; if not, the bound is wrong
            tol = np.zeros(U)
            Efull = np.full((U, P), np.nan)
            worst = 0.0
            for u in range(U):
                cands, s, E = no.user_row(params, BETA, indptr, indices, rate, region_of, u)
                assert not np.isnan(rows[u, cands]).any() and not np.isnan(s).any(), (tag, u)
                dev = np.abs(rows[u, cands].astype(np.float64) - s)
                assert np.all(dev <= E), (tag, u, float((dev / E).max()))
                worst = max(worst, float((dev / E).max()))
                tol[u] = 2.0 * E.max()
                Efull[u, cands] = E
            if tag == "init" or margins_ok(rows, Efull, val, test):
                break
        else:
            raise SystemExit("no seed with the margins")
        if tag == "sharp":
            sat = float(np.mean((rows == 1.0) | (rows == 0.0)))
            assert sat < 0.01, sat
            out["sharp/max_abs_logit"], out["sharp/saturated"] = np.float64(amax), np.float64(sat)
        print(tag, "seed", seed, "worst dev / E", worst, "max 2E", tol.max())
        out[f"{tag}/seed"] = np.int64(seed)
        for k, v in params.items():
            out[f"{tag}/{k}"] = v
        out[f"{tag}/rows"] = rows
        out[f"{tag}/topk_ids"] = np.array(recs["rec"], dtype=np.int64)
        out[f"{tag}/topk_scores"] = np.take_along_axis(rows, out[f"{tag}/topk_ids"], 1)
        out[f"{tag}/metrics"] = np.array(metrics, dtype=np.float64)
        if tag == "init":
            out["visit_rate_flat"] = np.concatenate(seen_rates)
        for (b, n), (hist, target, hreg, treg, vr) in fwd_in.items():
            with torch.no_grad():
                pred = m(torch.from_numpy(hist), torch.from_numpy(target), torch.from_numpy(hreg),
                         torch.from_numpy(treg), torch.from_numpy(vr))
            s, E = no.forward_rows(params, BETA, hist, target, hreg, treg, vr.astype(np.float32))
            assert np.all(np.abs(pred.numpy().astype(np.float64) - s) <= E), (tag, b, n)
            out[f"{tag}/fwd{b}x{n}/prediction"] = pred.numpy()

    # overflow: the spread parameters with attn_Q / attn_K scaled up; rows chosen by their logits
    params = {k: out["spread/" + k].copy() for k in no.NAMES}
    params["attn_Q.weight"] = (params["attn_Q.weight"] * np.float32(40.0)).astype(np.float32)
    params["attn_K.weight"] = (params["attn_K.weight"] * np.float32(40.0)).astype(np.float32)
    srng = np.random.default_rng(99)
    want = [lambda a: a.max() > 89.72 + 1 and a.max() < 1000, lambda a: a.max() < -111.0,
            lambda a: np.abs(a).max() < 60.0]
    picked = []
    for cond in want:
        for _ in range(200000):
            hist = srng.choice(P, 2, replace=False)
            c = int(srng.integers(0, P))
            if c in hist:
                continue
            a = no.logits(params, hist, region_of[hist], [c], region_of[[c]])[0]
            if cond(a) and np.all((np.abs(np.abs(a) - 88.72) > 1.0) & (np.abs(a + 103.97) > 1.0)):
                picked.append((hist, c))
                break
        else:
            raise SystemExit("no overflow row found")
    hist = np.stack([h for h, _ in picked]).astype(np.int64)
    target = np.array([c for _, c in picked], dtype=np.int64)
    vr = np.array([0.5, 0.25])
    m = model.New1(P, D, D, BETA, R)
    load_params(torch, m, params)
    m.eval()
    with torch.no_grad():
        pred = m(torch.from_numpy(hist), torch.from_numpy(target), torch.from_numpy(region_of[hist]),
                 torch.from_numpy(region_of[target]), torch.from_numpy(vr)).numpy()
    assert np.isnan(pred[0]) and np.isnan(pred[1]) and np.isfinite(pred[2]), pred
    s, E = no.forward_rows(params, BETA, hist, target, region_of[hist], region_of[target],
                           vr.astype(np.float32))
    assert np.array_equal(np.isnan(s), np.isnan(pred)) and abs(s[2] - pred[2]) <= E[2]
    for k, v in params.items():
        out["overflow/" + k] = v
    out["overflow/history"], out["overflow/target"] = hist, target
    out["overflow/history_region"], out["overflow/target_region"] = region_of[hist], region_of[target]
    out["overflow/visit_rate"], out["overflow/prediction"] = vr, pred

    path = os.path.join(HERE, "new1.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
