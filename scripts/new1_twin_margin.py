"""The margin of tests/test_gpu_new1_train.py::test_epoch_against_a_twin, measured on the CPU.

Steps New1.restatement + loss_func + torch.optim.Adam through the test's 12 batches (the fixture
of tests/golden/new1.npz, users 0..11, num_ng 4, the seeds the test's torch.manual_seed(5) draws,
the negatives the host model of the sampler predicts) once in float32 and once in float64 and
prints the two epoch losses and their relative difference. The test allows 4 x that difference:
the device's fused step and the device's twin both round differently from either CPU run.

Usage: python scripts/new1_twin_margin.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _new1_oracle as no  # noqa: E402
import _sampler_ref as sr  # noqa: E402
from _helpers import load_golden  # noqa: E402
from _new1_common import golden_params, make_model  # noqa: E402

USERS, NUM_NG, LR, WD = range(12), 4, 0.01, 1e-7


def main():
    z = load_golden("new1.npz")
    P, beta = int(z["num_pois"]), float(z["beta"])
    indptr, indices, region_of = z["indptr"], z["indices"], z["region_of"]
    rate = no.visit_rates(indptr, indices, z["data"], P)
    torch.manual_seed(5)
    seeds = [int(torch.randint(0, 2**62, (1,)).item()) for _ in USERS]
    losses = {}
    for dtype in (torch.float32, torch.float64):
        m = make_model(golden_params(z, "spread"), beta).to(dtype).train()
        opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WD)
        total = 0.0
        for u, seed in zip(USERS, seeds):
            row = indices[indptr[u]:indptr[u + 1]].astype(np.int64)
            n = len(row)
            neg = sr._first_free(row, P, n * NUM_NG, n * (NUM_NG + 1), sr.nais_seeds(seed)[1])
            tgt = np.concatenate([row[:, None], neg.reshape(n, NUM_NG)], 1).reshape(-1)
            lab = np.tile(np.array([1.0] + [0.0] * NUM_NG), n)
            b = len(tgt)
            vr = torch.from_numpy(rate[indptr[u]:indptr[u + 1]].astype(np.float32)).to(dtype)
            h = torch.from_numpy(row)
            opt.zero_grad()
            pred = m.restatement(h.expand(b, n), torch.from_numpy(tgt), torch.from_numpy(region_of[row]).expand(b, n),
                                 torch.from_numpy(region_of[tgt]), vr.to(torch.float32) if dtype == torch.float32 else vr)
            loss = m.loss_func(pred, torch.from_numpy(lab).to(dtype))
            loss.backward()
            opt.step()
            total += float(loss)
        losses[dtype] = total
    a, b = losses[torch.float32], losses[torch.float64]
    print(f"float32 twin {a:.12g}  float64 twin {b:.12g}  relative difference {abs(a - b) / abs(b):.3g}")


if __name__ == "__main__":
    main()
