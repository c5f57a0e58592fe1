"""Golden forwards of the table-based New4 family at the reference driver's widths, produced by
the REFERENCE's own classes on the CPU: New4 (model.py:1169), New4_padding (:1308), all_in_out
(:1447), nearPOI_embedding (:1578), no_POI_emb (:1707), transform_ingoing_outgoing (:1822),
transform_attn (:1959) and only_area_not_inout (:2100). Run here only:

    python tests/golden/make_golden_new4_family_wide.py [/root/reference]

Two configurations (embed_size, hidden, near POIs): "wide" = (128, 128, 50), the driver's
factor_num = hidden_dim = 128 (run_new.py:345-346) with near_POI_num = 50 (datasets.py:422), and
"odd" = (48, 40, 7), an embed_size off the scorer's native widths (12-wide pools, tables padded
to 64 on the device). As in make_golden_new4_family.py, torch.Tensor.cuda is the identity for the
run and every state_dict entry is overwritten with seeded values of its shape (embeddings
N(0, 0.3), Linear weights U(+-1/sqrt(in)), biases N(0, 0.1)).

Size: at E = H = 128 the Linear weights of the eight members alone are 1 MB of float32, so to
keep the file under 1 MiB the parameters are rounded to float16-representable values BEFORE the
reference runs and stored as float16 (the loader widens them back to the same float32 bits; the
reference computed with exactly those values), and the wide configuration has P = 90 POIs
(the odd one P = 100). No member is dropped.

new4_family_wide.npz   per configuration C in (wide, odd): C/near, C/shape = (P, E, H, K, R), and
                       per member M: C/M/<param> (float16), C/M/n{1,9}/{hist,target,pred}
                       (forward on [32, n] batches; row 0 has its target inside the history).
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import load_params, load_reference  # noqa: E402
from make_golden_new4 import near_pois  # noqa: E402
from make_golden_new4_family import random_state  # noqa: E402

MEMBERS = ("New4", "New4_padding", "all_in_out", "nearPOI_embedding", "no_POI_emb",
           "transform_ingoing_outgoing", "transform_attn", "only_area_not_inout")
CONFIGS = {"wide": (90, 128, 128, 50, 20), "odd": (100, 48, 40, 7, 20)}   # P, E, H, K, R


def main(ref_path="/root/reference"):
    import torch
    torch.set_num_threads(8)
    model = load_reference(ref_path)[0]
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        rng = np.random.default_rng(8642)
        out = {}
        for ci, (cfg, (P, E, H, K, R)) in enumerate(CONFIGS.items()):
            near = near_pois(P, K, 11 + ci)
            near[3, 1:4] = near[3, 0]          # repeated ids inside one near list
            out[f"{cfg}/near"] = near
            out[f"{cfg}/shape"] = np.array([P, E, H, K, R], np.int64)
            for mi, name in enumerate(MEMBERS):
                m = getattr(model, name)(P, E, H, 0.5, R)
                p16 = {k: v.astype(np.float16) for k, v in random_state(m, 900 + 20 * ci + mi).items()}
                load_params(torch, m, {k: v.astype(np.float32) for k, v in p16.items()})
                m.eval()
                out.update({f"{cfg}/{name}/{k}": v for k, v in p16.items()})
                for n in (1, 9):
                    b = 32
                    hist = np.stack([rng.choice(P, n, replace=False) for _ in range(b)]).astype(np.int64)
                    tgt = rng.integers(0, P, b).astype(np.int64)
                    tgt[0] = hist[0, 0]
                    with torch.no_grad():
                        pred = m(torch.from_numpy(hist), torch.from_numpy(tgt), near,
                                 torch.zeros(b, dtype=torch.int64)).numpy()
                    out[f"{cfg}/{name}/n{n}/hist"] = hist
                    out[f"{cfg}/{name}/n{n}/target"] = tgt
                    out[f"{cfg}/{name}/n{n}/pred"] = pred.astype(np.float32)
                print(cfg, name, "done", flush=True)
        path = os.path.join(HERE, "new4_family_wide.npz")
        np.savez_compressed(path, **out)
        print("written", path, os.path.getsize(path), "bytes")
    finally:
        torch.Tensor.cuda = orig_cuda


if __name__ == "__main__":
    main(*sys.argv[1:])
