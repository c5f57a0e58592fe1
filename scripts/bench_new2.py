"""Time one New2 evaluation job (new1.catalog_tables + new2.score_topk with `coords`: the catalog's
Q / K / V tables, then the fused scorer + top-50 of every user over the complement of its history,
every pair's haversine distance evaluated in float64 on the device) at the bench's config-2 and
config-4 geometry (d = 64, R = 1,024), beside
  the New1 job (new1.score_topk) on the same module, data and GPU in the same process -- the
  ratio is the price of the geo term -- and
  the torch restatement of the reference's loop on the same GPU: per user the [n, b] distance
  block built on the device in float64 (the reference slices a dense P x P float64 matrix, 80 GB
  at config 4), one `New2.restatement` call over all its candidates and torch.topk.

    python scripts/bench_new2.py [--config 2 4] [--dim 64] [--sample 6] [--out profiles/new2]

One JSON line per (config, dim): median ms of the fused New2 job and of the New1 job (HIP events;
one warm-up job, then --repeat timed jobs; a job is the whole call with its host-side visit rates
and uploads), the torch route's ms per sampled user (the users spread over the history lengths;
one warm-up each) scaled to all users by the work n_u C_u, the job's MFMA work
4 d sum_u n_u C_u FLOP with its floor at the 155 TF/s measured fp32 MFMA rate, the count of
float64 distance evaluations sum_u n_u C_u, and how the sampled users' lists compare.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = {2: dict(U=10_000, P=50_000, h_max=100), 4: dict(U=50_000, P=100_000, h_max=200)}
FP32_MFMA_RATE = 155e12
TOPK = 50
REGIONS = 1024
BOX = (35.5, 35.8, 139.5, 139.9)            # data.write_synthetic's Tokyo box


def timed_ms(fn, repeat):
    import torch
    out = fn()                                                  # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(repeat):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), times, out


def dist_block(rad, hist, cands):
    """[n, b] float64 kilometres on the device: new2.haversine_km in torch ops."""
    import torch
    from poi_recommendation_models_amd.new2 import EARTH_RADIUS_KM
    a, b = rad[hist], rad[cands]
    lat = b[None, :, 0] - a[:, None, 0]
    lng = b[None, :, 1] - a[:, None, 1]
    d = torch.sin(lat * 0.5) ** 2 + torch.cos(a[:, None, 0]) * torch.cos(b[None, :, 0]) * torch.sin(lng * 0.5) ** 2
    return 2 * EARTH_RADIUS_KM * torch.asin(torch.sqrt(d))


def run(config, d, repeat, sample, chunks=0):
    import torch
    from poi_recommendation_models_amd import new1, new2
    from poi_recommendation_models_amd.model import New2
    from poi_recommendation_models_amd.synthetic import make_checkins
    g = CONFIGS[config]
    U, P = g["U"], g["P"]
    data = make_checkins(U, P, g["h_max"], seed=config)
    X = data.to_scipy().tocsr()
    X.sort_indices()
    rng = np.random.default_rng(20 + config)
    X.data = rng.integers(1, 6, X.nnz).astype(np.float64)      # visit counts 1..5
    region_of = rng.integers(0, REGIONS, P).astype(np.int64)
    coords = np.stack([rng.uniform(BOX[0], BOX[1], P), rng.uniform(BOX[2], BOX[3], P)], 1)
    torch.manual_seed(config)
    m = New2(P, d, d, 0.5, REGIONS, U)
    with torch.no_grad():                                       # parameters at a trained scale
        m.embed_target.weight.normal_(0.0, 0.3)
        m.embed_region.weight.normal_(0.0, 0.3)
        m.embed_dist.normal_(0.0, 0.5)
    dev = torch.device("cuda:0")
    m = m.to(dev).eval()
    users = np.arange(U)
    new1_ms, new1_all, _ = timed_ms(
        lambda: new1.score_topk(m, X, region_of, users, TOPK, num_chunks=chunks), repeat)
    job_ms, job_all, (ids, _) = timed_ms(
        lambda: new2.score_topk(m, X, region_of, users, TOPK, coords=coords, num_chunks=chunks), repeat)

    # the torch route on a sample of users spread over the history lengths
    hl = np.diff(X.indptr)
    order = np.argsort(hl, kind="stable")
    picks = order[np.linspace(0, U - 1, sample).astype(np.int64)]
    _, r64 = new1.visit_rates(X)
    reg = torch.from_numpy(region_of).to(dev)
    rad = torch.deg2rad(torch.from_numpy(coords).to(dev))
    per_user, same, sets = [], 0, 0
    for u in picks:
        lo, hi = int(X.indptr[u]), int(X.indptr[u + 1])
        hist = torch.from_numpy(X.indices[lo:hi].astype(np.int64)).to(dev)
        cands = torch.from_numpy(np.setdiff1d(np.arange(P), X.indices[lo:hi])).to(dev)
        rate = torch.from_numpy(r64[lo:hi]).to(dev)

        def job():
            with torch.no_grad():
                s = m.restatement(hist.unsqueeze(0).expand(len(cands), -1), cands,
                                  reg[hist].unsqueeze(0).expand(len(cands), -1), reg[cands], rate,
                                  dist_block(rad, hist, cands), int(u))
                return cands[torch.topk(s, TOPK)[1]]
        ms, _, tids = timed_ms(job, 3)
        per_user.append(ms)
        same += int(torch.equal(tids, ids[u]))
        sets += int(torch.equal(torch.sort(tids)[0], torch.sort(ids[u])[0]))
    # scaled by the work: a user's torch time is proportional to n_u C_u
    work = hl.astype(np.float64) * (P - hl)
    torch_job_ms = float(np.sum(per_user) / work[picks].sum() * work.sum())
    flop = 4.0 * d * float(work.sum())
    return dict(bench="new2_eval", config=config, num_users=U, num_pois=P, dim=d, regions=REGIONS,
                topk=TOPK, h_max=g["h_max"], mean_history=float(hl.mean()), repeat=repeat,
                num_chunks=chunks, fused_job_ms=job_ms, fused_job_ms_all=job_all,
                new1_job_ms=new1_ms, new1_job_ms_all=new1_all, ratio_to_new1=job_ms / new1_ms,
                torch_sample_users=int(sample), torch_sample_history=[int(x) for x in hl[picks]],
                torch_ms_per_user=per_user, torch_median_ms_per_user=float(np.median(per_user)),
                torch_job_ms_scaled=torch_job_ms, speedup_vs_torch_scaled=torch_job_ms / job_ms,
                flop=flop, floor_ms=flop / FP32_MFMA_RATE * 1e3,
                fraction_of_fp32_mfma_rate=flop / (job_ms * 1e-3) / FP32_MFMA_RATE,
                distance_evaluations=float(work.sum()),
                ns_per_distance_evaluation=job_ms * 1e6 / float(work.sum()),
                sample_lists_equal_torch=same, sample_sets_equal_torch=sets)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, nargs="+", default=[2, 4], choices=sorted(CONFIGS))
    ap.add_argument("--dim", type=int, nargs="+", default=[64])
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--sample", type=int, default=6, help="users timed on the torch route")
    ap.add_argument("--chunks", type=int, default=0, help="column chunks of the fused kernel (0: its own choice)")
    ap.add_argument("--out", default=None, help="directory that receives config<N>.json")
    args = ap.parse_args()
    for c in args.config:
        lines = []
        for d in args.dim:
            lines.append(json.dumps(run(c, d, args.repeat, args.sample, args.chunks)))
            print(lines[-1], flush=True)
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, f"config{c}.json"), "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
