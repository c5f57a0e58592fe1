"""Full-catalog New2 evaluation on the device (the evaluation loop of run_new.py:551-570).

New2 is New1 plus a geographic weight per (candidate row, history item): the T / Q / K / V tables
are New1's (`new1.catalog_tables`), the visit rates New1's (`new1.visit_rates`), and
`nais_new2_score_topk` is New1's fused scorer + top-k with the geo term. The reference's
testDataset2 builds a dense P x P float64 haversine matrix and slices an [n, P - n] block of it
per user; here the distance of a pair is evaluated where it is used, from `coords`, in float64 in
the haversine formula's operation order (or read from a caller's dense float32 `dist_mat`, for
small catalogs and tests).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _capi
from .catalog import _user_array, device_csr
from .new1 import MAX_USERS_PER_CALL, _region_tensor, catalog_tables, visit_rates

EARTH_RADIUS_KM = 6371.0088      # the haversine package's mean radius


def haversine_km(a, b):
    """[len(a), len(b)] float64 kilometres between (lat, lng) rows in degrees: the haversine
    package's `haversine_vector(..., comb=True)` formula in its operation order (the matrix is
    symmetric for a == b, so its orientation does not matter there)."""
    a, b = np.radians(np.asarray(a, np.float64)), np.radians(np.asarray(b, np.float64))
    lat = b[None, :, 0] - a[:, None, 0]
    lng = b[None, :, 1] - a[:, None, 1]
    d = np.sin(lat * 0.5) ** 2 + np.cos(a[:, None, 0]) * np.cos(b[None, :, 0]) * np.sin(lng * 0.5) ** 2
    return 2 * EARTH_RADIUS_KM * np.arcsin(np.sqrt(d))


def score_topk(model, train_matrix, region_of, users, k, coords=None, dist_mat=None, num_chunks=0,
               tables=None):
    """Top-k (ids int64 [len(users), k], scores f32, best first) of every listed user over the
    complement of its training history, scored as the reference's evaluation batch of that user:
    all candidates in ascending POI id, one shared history in ascending POI id. The distances come
    from exactly one of `coords` ([P, 2] float64 (lat, lng), evaluated on the device) and
    `dist_mat` ([P, P], cast to float32); neither or both raise ValueError. Everything else --
    padding of short lists and `model._last_short`, the visit rates, `tables`, `num_chunks` -- as
    `new1.score_topk`. A user id is also the row of `embed_dist`."""
    dev = model._check_device()
    if (coords is None) == (dist_mat is None):
        raise ValueError("New2: give exactly one of coords and dist_mat")
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
    if n and (users.min() < 0 or users.max() >= min(csr.shape[0], model.embed_dist.shape[0])):
        raise IndexError("New2: user id out of range")
    co = dm = None
    if coords is not None:
        co = torch.as_tensor(np.ascontiguousarray(np.asarray(
            coords.cpu() if torch.is_tensor(coords) else coords, dtype=np.float64))).to(dev)
        if tuple(co.shape) != (P, 2):
            raise ValueError(f"coords must be [{P}, 2], got {tuple(co.shape)}")
    else:
        dm = torch.as_tensor(dist_mat).to(device=dev, dtype=torch.float32).contiguous()
        if tuple(dm.shape) != (P, P):
            raise ValueError(f"dist_mat must be [{P}, {P}], got {tuple(dm.shape)}")
    reg = _region_tensor(model, region_of, dev)
    T, Q, K, V = tables if tables is not None else catalog_tables(model, region_of)
    rate = torch.from_numpy(r64.astype(np.float32)).to(dev)
    ids = torch.empty(n, k, dtype=torch.int64, device=dev)
    top = torch.empty(n, k, dtype=torch.float32, device=dev)
    model._last_short = torch.zeros(1, dtype=torch.int32, device=dev)
    lib = _capi.load()
    st = _capi.stream_handle(dev)
    prm = model.new2_params()
    u_all = torch.from_numpy(users.astype(np.int32)).to(dev)
    for g0 in range(0, n, MAX_USERS_PER_CALL):
        m = min(MAX_USERS_PER_CALL, n - g0)
        keys = torch.empty(m, k, dtype=torch.int64, device=dev)
        cnt = torch.empty(m, dtype=torch.int32, device=dev)
        need = lib.nais_new2_score_topk_workspace_size(prm, m, k, int(num_chunks))
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        _capi.check(lib.nais_new2_score_topk(
            prm, T.data_ptr(), Q.data_ptr(), K.data_ptr(), V.data_ptr(), reg.data_ptr(),
            csr.indptr.data_ptr(), csr.indices.data_ptr(), rate.data_ptr(), _capi.ptr(co),
            _capi.ptr(dm), u_all[g0:g0 + m].data_ptr(), m, k, int(num_chunks), keys.data_ptr(),
            cnt.data_ptr(), ws.data_ptr(), ws.numel(), st), "nais_new2_score_topk")
        ids32 = torch.empty(m, k, dtype=torch.int32, device=dev)
        _capi.check(lib.nais_topk_keys_finish(
            keys.data_ptr(), cnt.data_ptr(), m, k, ids32.data_ptr(), top[g0:g0 + m].data_ptr(),
            model._last_short.data_ptr(), st), "nais_topk_keys_finish")
        ids[g0:g0 + m] = ids32
    return ids, top
