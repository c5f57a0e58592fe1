"""Time one GeoIE evaluation job (geoie.score_topk: pair rows -> power-law table -> catalog scorer
-> top-50) at the bench's config-2 and config-4 geometry, coordinates route.

    python scripts/bench_geoie.py [--config 2 4] [--out profiles/geoie]

One JSON line per config: ms per job (HIP events, after one warm-up job), (user, candidate) pairs
per second, the table kernel's and the scorer's busy time (events around every launch of the timed
job), the scorer's algorithmic rate 2 D sum_u h_u (P - h_u) FLOP over its busy time as a fraction
of the 157.3 TF fp32 MFMA figure, and an 8-user self-check against tests/_geoie_oracle.py. There is
no pass mark: these lines are the baseline later work is judged against.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CONFIGS = {2: dict(U=10_000, P=50_000, h_max=100), 4: dict(U=50_000, P=100_000, h_max=200)}
PEAK_FP32_MFMA = 157.3e12
D, TOPK = 64, 50


def self_check(model, X, data, params, a, b, users, ids, sc):
    """8 users: the job's lists equal a separate small call's, whose score rows agree with the
    oracle on the 50 winners and 200 sampled candidates, none of which beats the 50th winner."""
    import _geoie_oracle as go
    from poi_recommendation_models_amd import geoie
    rng = np.random.default_rng(1)
    ids8, sc8, rows = geoie.score_topk(model, X, users, TOPK, coords=data.place_coords, return_rows=True)
    ids8, sc8, rows = ids8.cpu().numpy(), sc8.cpu().numpy(), rows.cpu().numpy()
    same = bool(np.array_equal(ids8, ids) and np.array_equal(sc8, sc))
    worst, beaten = 0.0, 0
    for i, u in enumerate(users):
        hist = data.history(int(u))
        comp = np.setdiff1d(np.arange(data.num_pois), hist)
        pick = np.unique(np.concatenate([ids8[i], rng.choice(comp, 200, replace=False)]))
        dist = go.distance_rows(data.place_coords, pick, hist)
        ref = go.forward(params, a, b, np.full(len(pick), u), pick, hist, dist)
        worst = max(worst, float(np.max(np.abs(ref - rows[i, pick]))))
        others = ~np.isin(pick, ids8[i])
        beaten += int(np.sum(ref[others] > sc8[i, -1] + 1e-4))
    return dict(ok=bool(same and worst <= 1e-4 and beaten == 0), users=len(users),
                lists_equal_separate_call=same, max_abs_vs_oracle=worst, sampled_beating_kth=beaten)


def run(config):
    import torch
    from poi_recommendation_models_amd import geoie
    from poi_recommendation_models_amd.model import GeoIE
    from poi_recommendation_models_amd.synthetic import make_checkins
    g = CONFIGS[config]
    U, P = g["U"], g["P"]
    data = make_checkins(U, P, g["h_max"], seed=config)      # coordinates in the bench's 0.3 x 0.4 box
    X = data.to_scipy()
    rng = np.random.default_rng(10 + config)
    names = ("UserPreference.weight", "PoiPreference.weight", "GeoInfluence.weight",
             "GeoSusceptibility.weight")
    params = {n: (0.3 * rng.standard_normal((U if n.startswith("User") else P, D))).astype(np.float32)
              for n in names}
    a, b = 0.8, -0.9
    m = GeoIE(U, P, D, 4, a, b)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    m = m.to("cuda:0").eval()
    users = np.arange(U)
    geoie.score_topk(m, X, users, TOPK, coords=data.place_coords)          # warm-up
    torch.cuda.synchronize()
    ev = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ids, sc = geoie.score_topk(m, X, users, TOPK, coords=data.place_coords, events=ev)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    busy = {}
    for kind, s, e in ev:
        busy[kind] = busy.get(kind, 0.0) + s.elapsed_time(e)
    h = np.diff(data.indptr).astype(np.float64)
    pairs = float(np.sum(P - h))
    flop = 2.0 * D * float(np.sum(h * (P - h)))
    rate = flop / (busy["score"] * 1e-3)
    chk_users = np.linspace(0, U - 1, 8).astype(np.int64)
    chk = self_check(m, X, data, params, a, b, chk_users, ids.cpu().numpy()[chk_users],
                     sc.cpu().numpy()[chk_users])
    return dict(bench="geoie_eval", config=config, num_users=U, num_pois=P, dim=D, topk=TOPK,
                h_max=g["h_max"], distances="coords", ms_per_job=ms, pairs_per_s=pairs / (ms * 1e-3),
                table_busy_ms=busy.get("table", 0.0), scorer_busy_ms=busy["score"],
                topk_busy_ms=busy.get("topk", 0.0), launches=len(ev), scorer_flop=flop,
                scorer_tflops=rate / 1e12, scorer_fraction_of_fp32_mfma_peak=rate / PEAK_FP32_MFMA,
                self_check=chk)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, nargs="+", default=[2, 4], choices=sorted(CONFIGS))
    ap.add_argument("--out", default=None, help="directory that receives config<N>.json")
    args = ap.parse_args()
    for c in args.config:
        line = json.dumps(run(c))
        print(line, flush=True)
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, f"config{c}.json"), "w") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
