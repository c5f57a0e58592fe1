"""GeoIE training (train_GeoIE, run.py:687-715), one SGD step per user, timed on one GPU.

Synthetic check-ins at config-2 and config-4 sizes (P = 50k / D = 64 and P = 100k /
D = 128; h ~ U{1..200}, num_ng 4, distances from coordinates). Legs, per user, on the SAME device
and the SAME prebuilt batches (one JSON line per config):
  fused_step     GeoIETrainer.step: forward + loss_function + backward + SGD in one C-ABI call
  batch          GeoIETrainer.batch alone: get_GeoIE_batch on the device
  fused          batch + step, what GeoIETrainer.epoch runs per user
  torch          the parent route: grad-enabled GeoIE.forward + loss_function + backward() +
                 torch.optim.SGD.step() (run.py:705-715 on the device; its per-step host sync, the
                 isnan(...).item() of loss_function and loss.item(), included -- the batch is NOT:
                 the reference builds it on the host, which this leg leaves out in its favour)

Every leg is warmed on every batch shape, then timed over `--rounds` rounds in which the legs
alternate; a timed window is a host clock around passes over all users that ends in a device
synchronise (8 passes for the fused legs, so a window is a fraction of a second). The JSON holds
the median, minimum and maximum of the rounds.

Usage: python scripts/bench_geoie_train.py [--config 2 4] [--users 256] [--out-dir profiles/geoie]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from poi_recommendation_models_amd.model import GeoIE  # noqa: E402
from poi_recommendation_models_amd.synthetic import make_checkins  # noqa: E402
from poi_recommendation_models_amd.trainer import GeoIETrainer  # noqa: E402

CONFIGS = {2: dict(P=50_000, D=64), 4: dict(P=100_000, D=128)}
H_MAX, NUM_NG, LR = 200, 4, 0.01


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


def run(cfg, users, rounds, reps):
    P, D = CONFIGS[cfg]["P"], CONFIGS[cfg]["D"]
    data = make_checkins(users, P, H_MAX, seed=20 + cfg)
    X = data.to_scipy()
    torch.manual_seed(cfg)
    m = GeoIE(users, P, D, NUM_NG, 0.8, -0.9).to("cuda:0")
    twin = GeoIE(users, P, D, NUM_NG, 0.8, -0.9).to("cuda:0")
    twin.load_state_dict(m.state_dict())
    tr = GeoIETrainer(m, X, lr=LR, num_ng=NUM_NG, poi_coords=data.place_coords)
    uids = list(range(users))
    bts = [tuple(x.clone() for x in tr.batch(u, seed=1000 + u)) for u in uids]
    rows = float(np.mean([len(b[2]) for b in bts]))

    opt = torch.optim.SGD(twin.parameters(), lr=LR)
    twin.train()

    def parent(i):                                                # run.py:705-715
        uid, hist, tgt, lab, freq, dist = bts[i]
        opt.zero_grad()
        pred, w = twin(uid, tgt, hist.unsqueeze(0).expand(len(tgt), -1), freq, dist)
        ls = twin.loss_function(pred, lab.unsqueeze(1), w)
        ls.backward()
        ls.item()
        opt.step()

    legs = {"fused_step": (lambda i: tr._step_uid(uids[i], bts[i]), reps),
            "batch": (lambda u: tr.batch(u, seed=u), reps),
            "fused_batch_plus_step": (lambda u: tr._step_uid(u, tr.batch(u, seed=u)), reps),
            "torch_parent_step": (parent, 1)}
    for fn, _ in legs.values():      # every shape of the timed window once
        one_pass(fn, uids, 1)
    times = {k: [] for k in legs}
    for _ in range(rounds):          # the legs alternate, so drift hits them alike
        for k, (fn, r) in legs.items():
            times[k].append(one_pass(fn, uids, r))
    loss = tr.finish()
    med = {k: float(np.median(v)) for k, v in times.items()}
    return dict(config=cfg, num_pois=P, embed_dim=D, users=users, h_max=H_MAX, num_ng=NUM_NG,
                mean_rows_per_batch=rows, rounds=rounds, fused_passes_per_round=reps,
                ms_per_user={k: spread(v) for k, v in times.items()},
                speedup_step=round(med["torch_parent_step"] / med["fused_step"], 2),
                speedup_with_batch=round(med["torch_parent_step"] / med["fused_batch_plus_step"], 2),
                fused_loss_finite=bool(np.isfinite(loss)), device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--users", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8, help="passes over the users per round of a fused leg")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "geoie"))
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    for cfg in a.config:
        line = json.dumps(run(cfg, a.users, a.rounds, a.reps))
        print(line, flush=True)
        with open(os.path.join(a.out_dir, f"train_config{cfg}.json"), "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
