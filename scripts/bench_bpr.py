"""Time one BPR evaluation job (bpr.score_topk: fused exact-fp32 inner products + top-50 of every
user over the complement of its history) at the bench's config-2 and config-4 geometry, beside the
torch route on the same GPU: chunked embed_user[chunk] @ embed_item.T, history set to -inf,
torch.topk.

    python scripts/bench_bpr.py [--config 2 4] [--dim 64 128] [--out profiles/bpr]

One JSON line per (config, dim): median ms per job of each route (HIP events; one warm-up job
each, then --repeat timed jobs of each, the two routes alternating; a job is the whole call, the
fused one with its upload of the user list and its id copy, the torch one with its host reads of
the CSR offsets), the fused route's algorithmic rate 2 U P D FLOP over its time as a
fraction of the 155 TF/s measured fp32 MFMA rate, and how the two routes' lists compare (they
sum in different orders, so near-ties may swap; the fused route's exactness is the test-suite's
business).
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
TORCH_CHUNK_BYTES = 2 << 30


def alternate_ms(fns, repeat):
    """Median ms of each route, the routes timed in turn (a, b, a, b, ...) after one warm-up
    job each, so both see the same clocks and the same neighbours."""
    import torch
    outs = [fn() for fn in fns]                                # warm-up
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(repeat):
        for x, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            outs[x] = fn()
            e1.record()
            torch.cuda.synchronize()
            times[x].append(e0.elapsed_time(e1))
    return [float(np.median(t)) for t in times], times, outs


def torch_route(m, indptr, indices, U, P):
    """The comparison route, with its index tensors built outside the timed part."""
    import torch
    dev = m.embed_user.weight.device
    chunk = max(1, min(U, TORCH_CHUNK_BYTES // (4 * P)))
    rows = torch.from_numpy(np.repeat(np.arange(U), np.diff(indptr))).to(dev)
    cols = torch.from_numpy(indices).to(dev)
    ptr = indptr

    def job():
        out = []
        with torch.no_grad():
            for u0 in range(0, U, chunk):
                u1 = min(U, u0 + chunk)
                s = m.embed_user.weight[u0:u1] @ m.embed_item.weight.T
                a, b = int(ptr[u0]), int(ptr[u1])
                s[rows[a:b] - u0, cols[a:b]] = float("-inf")
                out.append(torch.topk(s, TOPK, dim=1)[1])
        return torch.cat(out)
    return job


def run(config, D, repeat, chunks=0):
    import torch
    from poi_recommendation_models_amd import bpr
    from poi_recommendation_models_amd.catalog import device_csr
    from poi_recommendation_models_amd.model import BPR
    from poi_recommendation_models_amd.synthetic import make_checkins
    g = CONFIGS[config]
    U, P = g["U"], g["P"]
    data = make_checkins(U, P, g["h_max"], seed=config)
    X = data.to_scipy()
    rng = np.random.default_rng(10 + config)
    m = BPR(U, P, D)
    m.load_state_dict({"embed_user.weight": torch.from_numpy((0.3 * rng.standard_normal((U, D))).astype(np.float32)),
                       "embed_item.weight": torch.from_numpy((0.3 * rng.standard_normal((P, D))).astype(np.float32))})
    m = m.to("cuda:0").eval()
    csr = device_csr(X, torch.device("cuda:0"))
    users = np.arange(U)
    (fused_ms, torch_ms), (fused_all, torch_all), ((ids, _), tids) = alternate_ms(
        [lambda: bpr.score_topk(m, csr, users, TOPK, num_chunks=chunks),
         torch_route(m, csr.host_indptr, csr.host_indices, U, P)], repeat)
    same_rows = float((ids == tids).all(1).float().mean().item())
    same_sets = float((torch.sort(ids, 1)[0] == torch.sort(tids, 1)[0]).all(1).float().mean().item())
    flop = 2.0 * U * P * D
    return dict(bench="bpr_eval", config=config, num_users=U, num_pois=P, dim=D, topk=TOPK,
                h_max=g["h_max"], repeat=repeat, num_chunks=chunks, fused_ms=fused_ms, fused_ms_all=fused_all,
                torch_ms=torch_ms, torch_ms_all=torch_all, speedup_vs_torch=torch_ms / fused_ms,
                flop=flop, floor_ms=flop / FP32_MFMA_RATE * 1e3,
                fraction_of_fp32_mfma_rate=flop / (fused_ms * 1e-3) / FP32_MFMA_RATE,
                lists_equal_torch=same_rows, sets_equal_torch=same_sets)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, nargs="+", default=[2, 4], choices=sorted(CONFIGS))
    ap.add_argument("--dim", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--chunks", type=int, default=0, help="column chunks of the fused kernel (0: its own choice)")
    ap.add_argument("--out", default=None, help="directory that receives config<N>.json")
    args = ap.parse_args()
    for c in args.config:
        lines = []
        for D in args.dim:
            lines.append(json.dumps(run(c, D, args.repeat, args.chunks)))
            print(lines[-1], flush=True)
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, f"config{c}.json"), "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
