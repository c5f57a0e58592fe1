"""Full-catalog New1 evaluation on the device (the user loop of validation.py:212-230).

In evaluation every row of a user's batch carries the same history (batches.py:355), so the
model's Q, K and V projections depend on the POI only: `catalog_tables` forms them once for the
catalog (`nais_new1_catalog_tables`), and `nais_new1_score_topk` scores every listed user against
every POI outside its training history from those tables and keeps the k best per user without
writing a score row. `nais_topk_keys_finish` turns its keys into ids and scores: torch.topk's order
on the sigmoid scores, NaN first, ties by ascending POI id.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _capi
from .catalog import _user_array, device_csr

MAX_USERS_PER_CALL = 1 << 20     # keys of one call: users x k x 8 bytes


def _region_tensor(model, region_of, dev):
    P, R = model.embed_target.weight.shape[0], model.embed_region.weight.shape[0]
    reg = np.asarray(region_of.cpu() if torch.is_tensor(region_of) else region_of).reshape(-1)
    if reg.shape[0] != P:
        raise ValueError(f"region_of has {reg.shape[0]} entries, model has {P} POIs")
    reg = reg.astype(np.int64)
    if P and (reg.min() < 0 or reg.max() >= R):
        raise IndexError("New1: region id out of range")
    return torch.from_numpy(reg).to(dev)


def catalog_tables(model, region_of):
    """(T, Q, K, V), each [P, d] float32 on the model's device: the concatenated rows
    T[p] = [embed_target[p] | embed_region[region_of[p]]] and their attn_Q / attn_K / attn_V
    projections (exact fp32). They hold the parameters' values at the time of the call."""
    dev = model._check_device()
    P, d = model.embed_target.weight.shape[0], model._width()
    reg = _region_tensor(model, region_of, dev)
    tabs = torch.empty(4, P, d, dtype=torch.float32, device=dev)
    _capi.check(_capi.load().nais_new1_catalog_tables(
        model.new1_params(), reg.data_ptr(), tabs[0].data_ptr(), tabs[1].data_ptr(),
        tabs[2].data_ptr(), tabs[3].data_ptr(), _capi.stream_handle(dev)), "nais_new1_catalog_tables")
    return tabs[0], tabs[1], tabs[2], tabs[3]


def visit_rates(train_matrix):
    """(X, r): the matrix as a CSR with ascending rows and r[e] = data[e] / colsum[indices[e]] per
    entry, float64 (batches.py:350-359: the column sums run over all users of the matrix)."""
    X = train_matrix.tocsr() if not hasattr(train_matrix, "indptr") else train_matrix
    if not X.has_sorted_indices:
        X = X.sorted_indices()
    colsum = np.asarray(X.sum(axis=0), dtype=np.float64).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.asarray(X.data, dtype=np.float64) / colsum[X.indices]
    return X, r


def score_topk(model, train_matrix, region_of, users, k, num_chunks=0, tables=None):
    """Top-k (ids int64 [len(users), k], scores f32, best first) of every listed user over the
    complement of its training history, the history taken in ascending POI order (the order of a
    canonical CSR row, which is what the reference's getrow(...).indices gives). A user with fewer
    than k candidates has its list padded with -1 / NaN; `model._last_short` holds the number of
    such users (a device tensor). The visit rates are formed on the host in float64, cast to
    float32 and uploaded once. `tables` = catalog_tables(...) of the CURRENT parameters may be
    passed to share them between calls; they are never cached on the module. `num_chunks` forces
    the number of column chunks (tests; 0: chosen from the shape)."""
    dev = model._check_device()
    X, r64 = visit_rates(train_matrix)
    csr = device_csr(X, dev)
    P = model.embed_target.weight.shape[0]
    if csr.shape[1] != P:
        raise ValueError(f"train_matrix has {csr.shape[1]} POIs, model has {P}")
    k = int(k)
    if not 1 <= k <= 256:
        raise ValueError(f"k must be 1..256, got {k}")
    users = _user_array(users)
    n = len(users)
    if n and (users.min() < 0 or users.max() >= csr.shape[0]):
        raise IndexError("New1: user id out of range")
    T, Q, K, V = tables if tables is not None else catalog_tables(model, region_of)
    rate = torch.from_numpy(r64.astype(np.float32)).to(dev)
    ids = torch.empty(n, k, dtype=torch.int64, device=dev)
    top = torch.empty(n, k, dtype=torch.float32, device=dev)
    model._last_short = torch.zeros(1, dtype=torch.int32, device=dev)
    lib = _capi.load()
    st = _capi.stream_handle(dev)
    prm = model.new1_params()
    u_all = torch.from_numpy(users.astype(np.int32)).to(dev)
    for g0 in range(0, n, MAX_USERS_PER_CALL):
        m = min(MAX_USERS_PER_CALL, n - g0)
        keys = torch.empty(m, k, dtype=torch.int64, device=dev)
        cnt = torch.empty(m, dtype=torch.int32, device=dev)
        need = lib.nais_new1_score_topk_workspace_size(prm, m, k, int(num_chunks))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        _capi.check(lib.nais_new1_score_topk(
            prm, T.data_ptr(), Q.data_ptr(), K.data_ptr(), V.data_ptr(), csr.indptr.data_ptr(),
            csr.indices.data_ptr(), rate.data_ptr(), u_all[g0:g0 + m].data_ptr(), m, k,
            int(num_chunks), keys.data_ptr(), cnt.data_ptr(), ws.data_ptr(), ws.numel(), st),
            "nais_new1_score_topk")
        ids32 = torch.empty(m, k, dtype=torch.int32, device=dev)
        _capi.check(lib.nais_topk_keys_finish(
            keys.data_ptr(), cnt.data_ptr(), m, k, ids32.data_ptr(), top[g0:g0 + m].data_ptr(),
            model._last_short.data_ptr(), st), "nais_topk_keys_finish")
        ids[g0:g0 + m] = ids32
    return ids, top
