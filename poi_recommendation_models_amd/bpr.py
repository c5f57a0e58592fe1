"""Full-catalog BPR evaluation on the device (the user loop of validation.py:138-147).

`nais_bpr_score_topk` scores every listed user against every POI outside its training history
(exact-fp32 MFMA inner products) and keeps the k best per user without writing a score row;
`nais_topk_keys_finish` turns its keys into ids and scores, torch.topk's order with ties by
ascending POI id.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _capi
from .catalog import _user_array, device_csr

MAX_USERS_PER_CALL = 1 << 20     # keys of one call: users x k x 8 bytes


def score_topk(model, train_matrix, users, k, num_chunks=0, return_keys=False):
    """Top-k (ids int64 [len(users), k], scores f32, best first) of every listed user over the
    complement of its training history. A user with fewer than k candidates has its list padded
    with -1 / NaN; `model._last_short` holds the number of such users (a device tensor).
    `num_chunks` forces the number of column chunks (tests; 0: chosen from the shape);
    `return_keys` adds the raw uint64 keys (as int64) and their counts."""
    dev = model._check_device()
    csr = device_csr(train_matrix, dev)
    P = model.POI_count
    if csr.shape[1] != P:
        raise ValueError(f"train_matrix has {csr.shape[1]} POIs, model has {P}")
    k = int(k)
    if not 1 <= k <= 256:
        raise ValueError(f"k must be 1..256, got {k}")
    users = _user_array(users)
    n = len(users)
    if n and (users.min() < 0 or users.max() >= min(csr.shape[0], model.user_num)):
        raise IndexError("BPR: user id out of range")
    ids = torch.empty(n, k, dtype=torch.int64, device=dev)
    top = torch.empty(n, k, dtype=torch.float32, device=dev)
    keys_all = torch.empty(n, k, dtype=torch.int64, device=dev) if return_keys else None
    cnt_all = torch.empty(n, dtype=torch.int32, device=dev) if return_keys else None
    model._last_short = torch.zeros(1, dtype=torch.int32, device=dev)
    lib = _capi.load()
    st = _capi.stream_handle(dev)
    prm = model.bpr_params()
    u_all = torch.from_numpy(users.astype(np.int32)).to(dev)
    for g0 in range(0, n, MAX_USERS_PER_CALL):
        m = min(MAX_USERS_PER_CALL, n - g0)
        keys = keys_all[g0:g0 + m] if return_keys else torch.empty(m, k, dtype=torch.int64, device=dev)
        cnt = cnt_all[g0:g0 + m] if return_keys else torch.empty(m, dtype=torch.int32, device=dev)
        need = lib.nais_bpr_score_topk_workspace_size(prm, m, k, int(num_chunks))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        _capi.check(lib.nais_bpr_score_topk(
            prm, csr.indptr.data_ptr(), csr.indices.data_ptr(), u_all[g0:g0 + m].data_ptr(), m, k,
            int(num_chunks), keys.data_ptr(), cnt.data_ptr(), ws.data_ptr(), ws.numel(), st),
            "nais_bpr_score_topk")
        ids32 = torch.empty(m, k, dtype=torch.int32, device=dev)
        _capi.check(lib.nais_topk_keys_finish(
            keys.data_ptr(), cnt.data_ptr(), m, k, ids32.data_ptr(), top[g0:g0 + m].data_ptr(),
            model._last_short.data_ptr(), st), "nais_topk_keys_finish")
        ids[g0:g0 + m] = ids32
    return (ids, top, keys_all, cnt_all) if return_keys else (ids, top)
