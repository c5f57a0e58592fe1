"""New1 training (train_NAIS_new, run_new.py:391-410), one Adam step per user, timed on one GPU.

Synthetic check-ins at the geometry scripts/bench_new1.py uses for config 2 and config 4 (P = 50k /
100k, d = 64, R = 1,024 regions): 256 users, n ~ U{2..200} history items, visit counts 1..5,
num_ng 4. Legs, per user, on the SAME device and the SAME prebuilt batches (one JSON line per
config):
  fused_step     New1Trainer.step: forward + BCELoss + backward + dense Adam in one C-ABI call
  batch          New1Trainer.batch alone: trainDataset.__getitem__ on the device
  fused          batch + step, what New1Trainer.epoch runs per user
  torch          the parent route: grad-enabled New1.forward (the torch restatement) + loss_func +
                 backward() + torch.optim.Adam.step() on the device (run_new.py:403-410). Left out
                 in its favour: the batch, which the reference builds on the host, and the
                 loss.item() host sync of run_new.py:408 (the loss is accumulated on the device).

Every leg is warmed on every batch shape, then timed over `--rounds` rounds in which the legs
alternate; a timed window is a host clock around passes over all users that ends in a device
synchronise (`--reps` passes for the fused legs, one for the torch leg). The JSON holds the median,
minimum and maximum of the rounds, in ms per user.

Usage: python scripts/bench_new1_train.py [--config 2 4] [--users 256] [--out-dir profiles/new1]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from poi_recommendation_models_amd.model import New1  # noqa: E402
from poi_recommendation_models_amd.trainer import New1Trainer  # noqa: E402

CONFIGS = {2: dict(P=50_000), 4: dict(P=100_000)}
DIM, REGIONS, N_MIN, N_MAX, NUM_NG, LR, WD = 64, 1024, 2, 200, 4, 0.01, 1e-7


def one_pass(fn, items, reps):
    """ms per item of `reps` passes over `items`; the window ends in a device synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        for it in items:
            fn(it)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (reps * len(items)) * 1e3


def spread(v):
    return dict(median=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4))


def checkins(users, P, seed):
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(P, int(n), replace=False)) for n in rng.integers(N_MIN, N_MAX + 1, users)]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int64)
    data = rng.integers(1, 6, len(indices)).astype(np.float64)
    return sp.csr_matrix((data, indices, indptr), shape=(users, P)), rng.integers(0, REGIONS, P).astype(np.int64)


def run(cfg, users, rounds, reps):
    P = CONFIGS[cfg]["P"]
    X, region_of = checkins(users, P, 20 + cfg)
    torch.manual_seed(cfg)
    m = New1(P, DIM, DIM, 0.5, REGIONS)
    with torch.no_grad():                                       # embeddings at a trained scale
        m.embed_target.weight.normal_(0.0, 0.3)
        m.embed_region.weight.normal_(0.0, 0.3)
    m = m.to("cuda:0")
    twin = New1(P, DIM, DIM, 0.5, REGIONS).to("cuda:0")
    twin.load_state_dict(m.state_dict())
    tr = New1Trainer(m, X, region_of, lr=LR, weight_decay=WD, num_ng=NUM_NG)
    uids = list(range(users))
    bts = [tuple(x.clone() for x in tr.batch(u, seed=1000 + u)) for u in uids]
    rows = float(np.mean([len(b[1]) for b in bts]))

    opt = torch.optim.Adam(twin.parameters(), lr=LR, weight_decay=WD)   # run_new.py:389
    twin.train()
    acc = torch.zeros((), device="cuda:0")

    def parent(i):                                                # run_new.py:403-410
        hist, tgt, lab, hreg, treg, vr = bts[i]
        b, n = tgt.numel(), hist.numel()
        opt.zero_grad()
        pred = twin(hist.expand(b, n), tgt, hreg.expand(b, n), treg, vr)
        ls = twin.loss_func(pred, lab)
        acc.add_(ls.detach())
        ls.backward()
        opt.step()

    legs = {"fused_step": (lambda i: tr.step(*bts[i]), reps),
            "batch": (lambda u: tr.batch(u, seed=u), reps),
            "fused_batch_plus_step": (lambda u: tr.step(*tr.batch(u, seed=u)), reps),
            "torch_parent_step": (parent, 1)}
    for fn, _ in legs.values():      # every shape of the timed window once
        one_pass(fn, uids, 1)
    times = {k: [] for k in legs}
    for _ in range(rounds):          # the legs alternate, so drift hits them alike
        for k, (fn, r) in legs.items():
            times[k].append(one_pass(fn, uids, r))
    loss = tr.finish()
    med = {k: float(np.median(v)) for k, v in times.items()}
    parent_min = min(times["torch_parent_step"])
    return dict(bench="new1_train", config=cfg, num_pois=P, embed_dim=DIM, regions=REGIONS, users=users,
                n_range=[N_MIN, N_MAX], num_ng=NUM_NG, mean_rows_per_batch=rows, rounds=rounds,
                fused_passes_per_round=reps, ms_per_user={k: spread(v) for k, v in times.items()},
                speedup_step=round(med["torch_parent_step"] / med["fused_step"], 2),
                speedup_with_batch=round(med["torch_parent_step"] / med["fused_batch_plus_step"], 2),
                fused_below_parent_min=bool(med["fused_step"] < parent_min
                                            and med["fused_batch_plus_step"] < parent_min),
                dense_adam_bytes_per_step=int(6 * 4 * (P * DIM // 2 + REGIONS * DIM // 2 + 3 * DIM * DIM)),
                fused_loss_finite=bool(np.isfinite(loss)), parent_loss_finite=bool(torch.isfinite(acc)),
                device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, nargs="+", default=[2, 4], choices=sorted(CONFIGS))
    ap.add_argument("--users", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4, help="passes over the users per round of a fused leg")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "new1"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_new1_train.py needs a GPU: a CPU run measures nothing")
    os.makedirs(a.out_dir, exist_ok=True)
    for cfg in a.config:
        line = json.dumps(run(cfg, a.users, a.rounds, a.reps))
        print(line, flush=True)
        with open(os.path.join(a.out_dir, f"train_config{cfg}.json"), "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
