"""Full-catalog GeoIE evaluation on the device (the per-user body of validation.py:187-191).

For a group of users: `nais_pair_rows` lists their distinct history POIs, `nais_geoie_table`
evaluates the power-law term f = a * d ** b once per (history POI, candidate) pair of a column
block, `nais_geoie_score` forms every user's score row from it (exact-fp32 MFMA), and
`nais_topk_rows` is torch.topk. Distances come from the POI coordinates (float64 powerLaw.dist on
the device, nothing P x P is allocated) or from a caller's `dist_mat` (run.py:40-46, uploaded once).
User groups and column blocks are sized from `catalog.usable_device_bytes`.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _capi
from .catalog import _user_array, _workspace, device_csr, usable_device_bytes

MEMORY_FRACTION = 0.6            # of the usable device memory: half score rows, half the table block
TABLE_BLOCK_BYTES = 4 << 30      # a table block beyond this gains nothing (one launch per block)


def _distance_source(dev, P, dist_mat, coords):
    """(coords [P, 2] f64, None) or (None, dist_mat [P, P] f64) on the device."""
    if coords is not None:
        cor = torch.as_tensor(np.ascontiguousarray(coords, dtype=np.float64)).to(dev)
        if tuple(cor.shape) != (P, 2):
            raise ValueError(f"poi_coords must be [{P}, 2], got {tuple(cor.shape)}")
        return cor, None
    if dist_mat is None:
        raise ValueError("GeoIE needs poi_coords or the reference's dist_mat")
    if isinstance(dist_mat, torch.Tensor):
        dm = dist_mat.to(device=dev, dtype=torch.float64).contiguous()
    else:
        dm = torch.as_tensor(np.ascontiguousarray(dist_mat, dtype=np.float64)).to(dev)
    if tuple(dm.shape) != (P, P):
        raise ValueError(f"dist_mat must be [{P}, {P}], got {tuple(dm.shape)}")
    return None, dm


def pair_table(model, items, col0, cols, dist_mat=None, coords=None):
    """F [len(items), cols] f32: a * d ** b of history POIs `items` x candidates [col0, col0 + cols)
    (`nais_geoie_table`)."""
    dev = model._check_device()
    P = model.POI_count
    cor, dm = _distance_source(dev, P, dist_mat, coords)
    it = torch.as_tensor(np.asarray(items, dtype=np.int64)).to(dev)
    out = torch.empty(len(it), cols, dtype=torch.float32, device=dev)
    _capi.check(_capi.load().nais_geoie_table(
        _capi.ptr(cor), _capi.ptr(dm), P, it.data_ptr(), len(it), col0, cols, float(model.a),
        float(model.b), out.data_ptr(), cols, _capi.stream_handle(dev)), "nais_geoie_table")
    return out


def score_topk(model, train_matrix, users, k, dist_mat=None, coords=None, block_cols=None,
               group_users=None, return_rows=False, events=None):
    """Top-k (ids int64 [len(users), k], scores f32, best first; torch.topk's order with ties by
    ascending POI id) of every listed user over the complement of its training history, and with
    `return_rows` the full score rows [len(users), P] (history POIs = -1) as a third result.

    `block_cols` / `group_users` force the column-block width and the users per group (tests);
    by default both come from the usable device memory. `events`: optional list that receives
    (kind, start, end) HIP events around every table / scorer launch."""
    dev = model._check_device()
    csr = device_csr(train_matrix, dev)
    P = model.POI_count
    if csr.shape[1] != P:
        raise ValueError(f"train_matrix has {csr.shape[1]} POIs, model has {P}")
    users = _user_array(users)
    n = len(users)
    hl = csr.hist_len[users] if n else np.zeros(0, np.int64)
    if np.any(hl == 0):   # the reference's reshape raises (model.py:798); no score is invented
        raise ValueError(f"GeoIE: empty history (user {int(users[np.argmax(hl == 0)])})")
    if np.any(P - hl < k):
        raise RuntimeError("selected index k out of range")       # torch.topk's error
    ids = torch.empty(n, k, dtype=torch.int64, device=dev)
    top = torch.empty(n, k, dtype=torch.float32, device=dev)
    all_rows = torch.empty(n, P, dtype=torch.float32, device=dev) if return_rows else None
    model._last_nan = torch.zeros(1, dtype=torch.int32, device=dev)
    if n == 0:
        return (ids, top, all_rows) if return_rows else (ids, top)
    lib = _capi.load()
    st = _capi.stream_handle(dev)
    torch_stream = torch.cuda.current_stream(dev)
    cor, dm = _distance_source(dev, P, dist_mat, coords)
    prm = model.geoie_params()
    budget = int(usable_device_bytes(dev) * MEMORY_FRACTION)
    G = int(group_users) if group_users else max(1, min(n, (budget // 2) // (4 * P)))
    rowmap = torch.empty(P, dtype=torch.int32, device=dev)
    items = torch.empty(P, dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = _workspace(dev, lib.nais_pair_rows_workspace_size(P))
    short = torch.zeros(1, dtype=torch.int32, device=dev)
    u_all = torch.from_numpy(users.astype(np.int32)).to(dev)

    def timed(kind, fn):
        if events is None:
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch_stream)
        fn()
        e1.record(torch_stream)
        events.append((kind, e0, e1))

    for g0 in range(0, n, G):
        m = min(G, n - g0)
        u_dev = u_all[g0:g0 + m]
        _capi.check(lib.nais_pair_rows(csr.indptr.data_ptr(), csr.indices.data_ptr(), u_dev.data_ptr(),
                                       m, P, rowmap.data_ptr(), items.data_ptr(), cnt.data_ptr(),
                                       ws.data_ptr(), ws.numel(), st), "nais_pair_rows")
        J = int(cnt.item())
        rows = all_rows[g0:g0 + m] if return_rows else torch.empty(m, P, dtype=torch.float32, device=dev)
        cw = int(block_cols) if block_cols else \
            max(1, min(P, min(budget // 2, TABLE_BLOCK_BYTES) // (4 * max(J, 1))))
        cw = min(cw, P)
        tab = torch.empty(J, cw, dtype=torch.float32, device=dev)
        for c0 in range(0, P, cw):
            w = min(cw, P - c0)
            timed("table", lambda: _capi.check(lib.nais_geoie_table(
                _capi.ptr(cor), _capi.ptr(dm), P, items.data_ptr(), J, c0, w, float(model.a),
                float(model.b), tab.data_ptr(), cw, st), "nais_geoie_table"))
            timed("score", lambda: _capi.check(lib.nais_geoie_score(
                prm, csr.indptr.data_ptr(), csr.indices.data_ptr(), u_dev.data_ptr(), m,
                rowmap.data_ptr(), tab.data_ptr(), cw, J, c0, w, rows.data_ptr(), P, 0,
                model._last_nan.data_ptr(), st), "nais_geoie_score"))
        ids32 = torch.empty(m, k, dtype=torch.int32, device=dev)
        timed("topk", lambda: _capi.check(lib.nais_topk_rows(
            rows.data_ptr(), P, P, m, k, ids32.data_ptr(), top[g0:g0 + m].data_ptr(), short.data_ptr(),
            st), "nais_topk_rows"))
        ids[g0:g0 + m] = ids32
    return (ids, top, all_rows) if return_rows else (ids, top)
