"""Capture the BPR fixture from the reference itself (run HERE only; never on the GPU box).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_bpr.py REFERENCE_DIR
(REFERENCE_DIR = a checkout of muyeon-jo/POI_recommendation_models)

Writes tests/golden/bpr.npz: seeded CSR histories (h in 0..60, one user with none), two
parameter sets -- `init`, the reference's own N(0, 0.01) initialisation, and `spread`, N(0, 0.3)
-- and what the reference computes from them:
  model.BPR.forward (model.py:603-620) on n = 1, 7, 33 triples,
  validation.BPR_validation (validation.py:133-153): every user's candidate score row, the
  recommended top-50 lists with their scores, the 6-tuple,
  one get_BPR_batch training batch of 6 users (batches.py:6-22): predictions, the loss of
  run.py:506, the dense .grad of both tables, the tables after torch.optim.SGD(lr=0.01) at
  weight_decay 0 (the touched rows only: the others are asserted bit-identical) and 1e-3,
  and a 3-triple `saturated` batch on the spread tables with a few rows overwritten so that
  x = -200 for two triples: sigmoid rounds to 0, the loss is inf, their rows' gradients NaN.

Separation: the script asserts, and takes the next seed of a tag until it holds, that for every
user and every rank 1..50 the gap to the next reference score exceeds 2 * max_c E(u, c)
(tests/_bpr_oracle.py). The reference's list is then the only admissible one.
"""
from __future__ import annotations

import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import Args, load_params, load_reference  # noqa: E402
import _bpr_oracle as bo  # noqa: E402

P, D, U = 700, 16, 40
K_LIST = [5, 10, 15, 20, 25, 30]
TRAIN_USERS = [3, 7, 12, 18, 25, 33]
LR = 0.01


def make_inputs():
    rng = np.random.default_rng(2025)
    hl = rng.integers(1, 60, U)
    hl[0], hl[5], hl[9] = 0, 60, 1
    indptr, indices = [0], []
    for h in hl:
        indices.extend(np.sort(rng.choice(P, int(h), replace=False)).tolist())
        indptr.append(len(indices))
    indptr, indices = np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int64)
    val, test = [], []
    for u in range(U):
        comp = np.setdiff1d(np.arange(P), indices[indptr[u]:indptr[u + 1]])
        pick = rng.choice(comp, 12, replace=False)
        val.append([int(x) for x in pick[:5]])
        test.append([int(x) for x in pick[5:]])
    return indptr, indices, val, test


def separated(torch, m, indptr, indices):
    """The separation condition on the reference's own fp32 scores."""
    eu, ei = m.embed_user.weight.detach(), m.embed_item.weight.detach()
    tol = 2.0 * bo.E(eu.numpy(), ei.numpy()).max(1)
    for u in range(U):
        s = (eu[u].unsqueeze(0) * ei).sum(-1).numpy().astype(np.float64)
        s[indices[indptr[u]:indptr[u + 1]]] = -np.inf
        top = np.sort(s)[::-1][:51]
        if not np.all(top[:-1] - top[1:] > tol[u]):
            return False
    return True


def main(ref_path):
    import scipy.sparse as sp
    import torch
    torch.set_num_threads(4)
    model, validation, powerLaw, eval_metrics, run = load_reference(ref_path)
    import batches

    indptr, indices, val, test = make_inputs()
    X = sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(U, P))
    out = dict(indptr=indptr, indices=indices, num_pois=np.int64(P), num_users=np.int64(U),
               embed_dim=np.int64(D), k_list=np.array(K_LIST, dtype=np.int64),
               val_flat=np.array(sum(val, []), dtype=np.int64),
               val_len=np.array([len(x) for x in val], dtype=np.int64),
               test_flat=np.array(sum(test, []), dtype=np.int64),
               test_len=np.array([len(x) for x in test], dtype=np.int64))

    prng = np.random.default_rng(7)
    for tag in ("init", "spread"):
        for seed in range(100000):
            torch.manual_seed(seed)
            m = model.BPR(U, P, D)                                     # the reference's N(0, 0.01)
            if tag == "spread":
                srng = np.random.default_rng(seed)
                load_params(torch, m, {k: (0.3 * srng.standard_normal(tuple(v.shape))).astype(np.float32)
                                       for k, v in m.state_dict().items()})
            if separated(torch, m, indptr, indices):
                break
        else:
            raise SystemExit("no separated seed")
        out[f"{tag}/seed"] = np.int64(seed)
        params = {k: v.numpy().copy() for k, v in m.state_dict().items()}
        for k, v in params.items():
            out[f"{tag}/{k}"] = v
        m.eval()

        for n in (1, 7, 33):
            u = torch.from_numpy(prng.integers(0, U, n))
            i = torch.from_numpy(prng.integers(0, P, n))
            j = torch.from_numpy(prng.integers(0, P, n))
            with torch.no_grad():
                pi, pj = m(u, i, j)
            pre = f"{tag}/fwd{n}/"
            out[pre + "user"], out[pre + "item_i"], out[pre + "item_j"] = u.numpy(), i.numpy(), j.numpy()
            out[pre + "prediction_i"], out[pre + "prediction_j"] = pi.numpy(), pj.numpy()

        # the full validation: score rows through a forward hook, lists through evaluate_mp
        rows = np.full((U, P), np.nan, dtype=np.float32)            # history POIs stay NaN
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
                metrics = validation.BPR_validation(m, Args(), U, test, val, X, K_LIST)
        finally:
            validation.eval_metrics.evaluate_mp = orig
            hook.remove()
        out[f"{tag}/rows"] = rows
        out[f"{tag}/topk_ids"] = np.array(recs["rec"], dtype=np.int64)
        out[f"{tag}/topk_scores"] = np.take_along_axis(rows, out[f"{tag}/topk_ids"], 1)
        out[f"{tag}/metrics"] = np.array(metrics, dtype=np.float64)
        # the separation condition, on the captured rows
        tol = 2.0 * bo.E(params["embed_user.weight"], params["embed_item.weight"]).max(1)
        for u in range(U):
            s = np.sort(np.where(np.isnan(rows[u]), -np.inf, rows[u]).astype(np.float64))[::-1][:51]
            assert np.all(s[:-1] - s[1:] > tol[u]), (tag, u)
            assert np.array_equal(s[:50], out[f"{tag}/topk_scores"][u].astype(np.float64)), (tag, u)

        # one training batch as get_BPR_batch lays it out (shuffled triples of 6 users)
        random.seed(11)
        user, item_i, item_j = batches.get_BPR_batch(X, P, TRAIN_USERS)
        ii, jj = set(item_i.tolist()), set(item_j.tolist())
        assert len(ii) < len(item_i) and len(jj) < len(item_j) and ii & jj, "no repeated items"
        pre = f"{tag}/train/"
        out[pre + "user"], out[pre + "item_i"], out[pre + "item_j"] = user.numpy(), item_i.numpy(), item_j.numpy()
        for wd, name in ((0.0, "wd0"), (1e-3, "wd1e-3")):
            load_params(torch, m, params)
            m.train()
            opt = torch.optim.SGD(m.parameters(), lr=LR, weight_decay=wd)
            opt.zero_grad()
            pi, pj = m(user, item_i, item_j)
            loss = - (pi - pj).sigmoid().log().sum()                   # run.py:506
            loss.backward()
            if wd == 0.0:
                out[pre + "prediction_i"], out[pre + "prediction_j"] = pi.detach().numpy(), pj.detach().numpy()
                out[pre + "loss"] = np.float32(loss.item())
                for k, v in m.named_parameters():
                    out[pre + "grad/" + k] = v.grad.numpy().copy()
            opt.step()
            for k, v in m.state_dict().items():
                new = v.numpy().copy()
                if wd == 0.0:   # only the touched rows moved: store those (the rest is `params`)
                    rows = np.flatnonzero(np.any(new.view(np.int32) != params[k].view(np.int32), 1))
                    ids = user.numpy() if k.startswith("embed_user") else np.concatenate(
                        [item_i.numpy(), item_j.numpy()])
                    assert set(rows.tolist()) <= set(ids.tolist())
                    rows = np.unique(ids)
                    out[pre + name + "/rows/" + k], out[pre + name + "/" + k] = rows, new[rows]
                else:
                    out[pre + name + "/" + k] = new
        load_params(torch, m, params)

    # saturated: the spread tables with a few rows overwritten so that x = -200 twice
    sat = {k: out["spread/" + k].copy() for k in ("embed_user.weight", "embed_item.weight")}
    urow = np.zeros(D, np.float32)
    urow[0] = 10.0
    lo, hi = np.zeros(D, np.float32), np.zeros(D, np.float32)
    lo[0], hi[0] = -10.0, 10.0
    sat["embed_user.weight"][4] = urow
    sat["embed_item.weight"][[100, 101]] = lo
    sat["embed_item.weight"][[200, 201]] = hi
    user = torch.tensor([4, 8, 4])
    item_i = torch.tensor([100, 300, 101])
    item_j = torch.tensor([200, 301, 201])
    m = model.BPR(U, P, D)
    load_params(torch, m, sat)
    m.train()
    opt = torch.optim.SGD(m.parameters(), lr=LR)
    opt.zero_grad()
    pi, pj = m(user, item_i, item_j)
    loss = - (pi - pj).sigmoid().log().sum()
    loss.backward()
    assert np.isinf(loss.item()) and float((pi - pj)[0]) == -200.0
    pre = "saturated/"
    out[pre + "user_rows"], out[pre + "item_rows"] = np.array([4]), np.array([100, 101, 200, 201])
    out[pre + "user_values"] = sat["embed_user.weight"][[4]]
    out[pre + "item_values"] = sat["embed_item.weight"][[100, 101, 200, 201]]
    out[pre + "user"], out[pre + "item_i"], out[pre + "item_j"] = user.numpy(), item_i.numpy(), item_j.numpy()
    out[pre + "prediction_i"], out[pre + "prediction_j"] = pi.detach().numpy(), pj.detach().numpy()
    out[pre + "loss"] = np.float32(loss.item())
    tu, ti = np.array([4, 8]), np.array([100, 101, 200, 201, 300, 301])
    out[pre + "touched_users"], out[pre + "touched_items"] = tu, ti
    out[pre + "grad/embed_user.weight"] = m.embed_user.weight.grad.numpy()[tu].copy()
    out[pre + "grad/embed_item.weight"] = m.embed_item.weight.grad.numpy()[ti].copy()
    assert np.isnan(out[pre + "grad/embed_user.weight"][0]).all()
    opt.step()
    out[pre + "wd0/embed_user.weight"] = m.embed_user.weight.detach().numpy()[tu].copy()
    out[pre + "wd0/embed_item.weight"] = m.embed_item.weight.detach().numpy()[ti].copy()

    path = os.path.join(HERE, "bpr.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; seeds", out["init/seed"], out["spread/seed"])


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
