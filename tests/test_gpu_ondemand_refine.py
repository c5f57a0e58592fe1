"""GPU: the 3-product bound + on-demand exact refine form of the bounded route
(catalog.PAIR_ONDEMAND_REFINE; include/nais.h nais_pair_table_bound / nais_pair_scales /
nais_pair_bound_topk_widened / nais_pair_refine_topk_exact / nais_pair_recompute).

1. Pair bits: every recomputed (e, e*s) equals the fp16x6 pair table's bits for that (row, column)
   -- across 128-row groups, full chunks and a chunk tail, partial last tiles with the clamp to row
   P - 1, several table blocks of one job, and embedding rows whose magnitudes differ by 10^5 so
   that neighbouring chunks and tiles get different scales.
2. Bound validity: the hi words of the 3-product table, widened by catalog.ondemand_widening's
   (eta', delta_s), contain the fp16x6 values of every pair; the hi words are those of
   nais_pair_table_split at fp16x3. Prints the largest observed share of eta' and delta_s.
3. Route equality: ids, score bits and NaN counts of the new route equal the exact route's
   (PAIR_BOUNDED off) and the split16 route's (PAIR_ONDEMAND_REFINE off) on whole jobs.
4. Two gloo ranks on one GPU through sharding.distributed_topk_pairs give the single-process lists,
   each rank on the new route.
5. The widening cache (catalog.ondemand_widening) follows every writer of the parameters: in-place
   ops, load_state_dict, optim.Adagrad and NAISTrainer."""
import os
import socket
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _model(P, D, H, seed=3, emb_std=0.3, beta=0.5, spread=False):
    from poi_recommendation_models_amd import model as M
    from poi_recommendation_models_amd.synthetic import init_nais_params
    m = M.NAIS_basic(P, D, H, beta)
    p = init_nais_params(P, D, H, seed=seed, emb_std=emb_std, bias_std=0.1)
    if spread:   # per-row factors 1e-3 .. 1e2: chunks and tiles get different power-of-two scales
        rng = np.random.default_rng(seed + 100)
        for name in ("embed_history.weight", "embed_target.weight"):
            p[name] = (p[name] * 10.0 ** rng.uniform(-3, 2, (P, 1))).astype(np.float32)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()}, strict=False)
    m.precision = "fp16x6"
    m.report_nan = False
    return m.to(DEV).eval()


def _tables(m, items, c0, w, W, precision="fp16x6"):
    """(e, e*s) float tables [J, w] of nais_pair_table at `precision`, as uint32 bits."""
    from poi_recommendation_models_amd import _capi
    lib, J = _capi.load(), len(items)
    old, m.precision = m.precision, precision
    try:
        prm = m._score_params()
        f = torch.zeros(2, J, W, dtype=torch.float32, device=DEV)
        _capi.check(lib.nais_pair_table(prm, items.data_ptr(), J, c0, w, None, None, None, f[0].data_ptr(),
                                        f[1].data_ptr(), W, None, None), "nais_pair_table")
        torch.cuda.synchronize()
    finally:
        m.precision = old
    return f[:, :, :w].cpu().numpy()


def _scales(m, items, col0, cols, W):
    from poi_recommendation_models_amd import _capi
    J = len(items)
    rowsc = torch.zeros(J, 2, dtype=torch.float32, device=DEV)
    colsc = torch.zeros(cols, dtype=torch.float32, device=DEV)
    _capi.check(_capi.load().nais_pair_scales(m._score_params(), items.data_ptr(), J, col0, cols, W,
                                              rowsc.data_ptr(), colsc.data_ptr(), None), "nais_pair_scales")
    return rowsc, colsc


def _recompute(m, items, rowsc, colsc, col0, cols, rows, columns):
    from poi_recommendation_models_amd import _capi
    r = torch.as_tensor(rows, dtype=torch.int32, device=DEV)
    c = torch.as_tensor(columns, dtype=torch.int64, device=DEV)
    out = torch.zeros(2, len(rows), len(columns), dtype=torch.float32, device=DEV)
    _capi.check(_capi.load().nais_pair_recompute(
        m._score_params(), items.data_ptr(), len(items), rowsc.data_ptr(), colsc.data_ptr(), col0, cols,
        r.data_ptr(), len(rows), c.data_ptr(), len(columns), out[0].data_ptr(), out[1].data_ptr(), None),
        "nais_pair_recompute")
    torch.cuda.synchronize()
    return out.cpu().numpy()


P_T, J_T, W_T = 3000, 300, 512


def _items():
    # 300 rows: two full 128-row groups and a 44-row one (a full chunk and a 12-row tail); POIs
    # 5 .. 304 lie inside the first column block, so item == candidate pairs (e = 0) occur
    return torch.arange(5, 5 + J_T, dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("D,H", [(64, 64), (32, 32), (64, 32), (32, 64), (50, 40)])
def test_recomputed_pairs_equal_the_fp16x6_table_bits(D, H):
    m = _model(P_T, D, H, emb_std=0.01, spread=True)
    items = _items()
    rng = np.random.default_rng(D + H)
    rows = rng.permutation(J_T)           # any order: a pair's bits do not depend on its neighbours
    for c0 in (0, 700, P_T - 200):        # single-block jobs; the last is 200 wide (tiles of 32: 6.25)
        w = min(W_T, P_T - c0)
        f = _tables(m, items, c0, w, W_T).view(np.uint32)
        rowsc, colsc = _scales(m, items, c0, w, W_T)
        cols = c0 + rng.permutation(w)
        got = _recompute(m, items, rowsc, colsc, c0, w, rows, cols).view(np.uint32)
        np.testing.assert_array_equal(got[0], f[0][rows][:, cols - c0])     # e: every pair
        np.testing.assert_array_equal(got[1], f[1][rows][:, cols - c0])     # e * s
        if c0 == 0:   # the item == candidate pairs are in this block: e = +0
            assert not f[0][np.arange(J_T), 5 + np.arange(J_T)].any()
    # one job of several blocks: columns [100, P), blocks of 512 from 100; the last is 340 wide
    col0, NC = 100, P_T - 100
    rowsc, colsc = _scales(m, items, col0, NC, W_T)
    for c0 in (col0, col0 + 2 * W_T, col0 + 5 * W_T):
        w = min(W_T, P_T - c0)
        f = _tables(m, items, c0, w, W_T).view(np.uint32)
        cols = c0 + np.arange(w)
        got = _recompute(m, items, rowsc, colsc, col0, NC, np.arange(J_T), cols).view(np.uint32)
        np.testing.assert_array_equal(got[0], f[0])
        np.testing.assert_array_equal(got[1], f[1])


@pytest.mark.parametrize("D,H,spread", [(64, 64, True), (32, 32, True), (64, 64, False), (32, 32, False)])
def test_widened_hi_words_bound_the_fp16x6_values(D, H, spread):
    """For every pair: e in [e^ (1 - eta'), e^ (1 + 2^-7)(1 + eta')] and |e s - es~| within the
    widened radius of one term (nais_pairs.hip make_bounds), e^ / es~ from the 3-product hi word.
    Without the spread (trained-like N(0, 0.3) rows) the model is inside the route's gate, so the
    interval checked is the one the gather applies; the spread models (rows up to 10^2 times larger,
    eta' above the gate: such a model keeps the split16 route) check the derivation where its
    terms are largest."""
    from poi_recommendation_models_amd import _capi, catalog
    m = _model(P_T, D, H, emb_std=0.01 if spread else 0.3, spread=spread)
    lib = _capi.load()
    items = _items()
    _, eta, ds = catalog.ondemand_widening(m)
    assert np.isfinite(eta) and np.isfinite(ds) and eta < 2.0 ** -6, (eta, ds)   # not a vacuous interval
    assert spread or eta <= catalog.PAIR_ONDEMAND_ETA_MAX, eta                   # the gather would use it
    eta2 = 1.02 * eta + 2.0 ** -21
    share_eta = share_ds = 0.0
    for c0 in (0, 700, P_T - 200):
        w = min(W_T, P_T - c0)
        hi = torch.zeros(J_T, W_T, dtype=torch.int32, device=DEV)
        _capi.check(lib.nais_pair_table_bound(m._score_params(), items.data_ptr(), J_T, c0, w, None, None, None,
                                              hi.data_ptr(), W_T, None), "nais_pair_table_bound")
        m.precision = "fp16x3"
        hi3 = torch.zeros(J_T, W_T, dtype=torch.int32, device=DEV)
        ex3 = torch.zeros(J_T, 2 * W_T, dtype=torch.int32, device=DEV)
        _capi.check(lib.nais_pair_table_split(m._score_params(), items.data_ptr(), J_T, c0, w, None, None, None,
                                              hi3.data_ptr(), ex3.data_ptr(), W_T, None, None), "table_split")
        m.precision = "fp16x6"
        torch.cuda.synchronize()
        hw = hi.cpu().numpy().view(np.uint32)[:, :w]
        np.testing.assert_array_equal(hw, hi3.cpu().numpy().view(np.uint32)[:, :w])   # split16's hi at fp16x3
        e6, es6 = (t.astype(np.float64) for t in _tables(m, items, c0, w, W_T))
        e3, es3 = (t.astype(np.float64) for t in _tables(m, items, c0, w, W_T, "fp16x3"))
        eh = (hw << 16).view(np.float32).astype(np.float64)           # e^: e~ truncated to 16 bits
        esw = hw.view(np.float32).astype(np.float64)                  # es~: the word as the gather reads it
        tiny = 2.0 ** -126
        assert np.all(e6 >= eh * (1 - eta) - tiny)
        assert np.all(e6 <= eh * (1 + 2.0 ** -7) * (1 + eta) + tiny)
        radius = (2.0 ** -7 + eta2) * np.abs(esw) + eh * (1 + 2.0 ** -7) * (1 + eta) * ds + tiny
        assert np.all(np.abs(es6 - esw) <= radius)
        ok = (e6 > 2.0 ** -100) & (e3 > 2.0 ** -100)
        share_eta = max(share_eta, float(np.abs(np.log(e3[ok] / e6[ok])).max() / eta))
        share_ds = max(share_ds, float(np.abs(es3[ok] / e3[ok] - es6[ok] / e6[ok]).max() / ds))
    print("D=%d H=%d spread=%s eta'=%.3e (gate 2^-9: %s) delta_s=%.3e largest observed share: eta %.2e delta_s %.2e"
          % (D, H, spread, eta, "inside" if eta <= catalog.PAIR_ONDEMAND_ETA_MAX else "outside", ds,
             share_eta, share_ds))
    assert share_eta <= 1.0 and share_ds <= 1.0


def _run(m, data, k, route, users=None, cols=None):
    """route: "ondemand", "split16" (PAIR_ONDEMAND_REFINE off) or "exact" (PAIR_BOUNDED off)."""
    from poi_recommendation_models_amd import catalog
    from poi_recommendation_models_amd.catalog import DeviceCSR, _score_topk_pairs
    csr = DeviceCSR.from_arrays(data.indptr, data.indices, data.num_pois, DEV)
    users = np.arange(data.num_users) if users is None else users
    old = catalog.PAIR_BOUNDED, catalog.PAIR_ONDEMAND_REFINE
    catalog.PAIR_BOUNDED, catalog.PAIR_ONDEMAND_REFINE = route != "exact", route == "ondemand"
    try:
        ev = []
        ids, sc = _score_topk_pairs(m, csr, users, k, None, None, None, None, force=True, cols=cols, events=ev)
    finally:
        catalog.PAIR_BOUNDED, catalog.PAIR_ONDEMAND_REFINE = old
    torch.cuda.synchronize()
    took = [v for kind, _, _, v in ev if kind == "pair_route"]
    return ids.cpu().numpy(), sc.cpu().numpy(), int(m._last_nan.item()), took


def _same_three(m, data, k, **kw):
    new, old, exact = (_run(m, data, k, r, **kw) for r in ("ondemand", "split16", "exact"))
    assert new[3] == ["ondemand"] and old[3] == ["split16"] and exact[3] == ["exact"], (new[3], old[3], exact[3])
    for ref in (exact, old):
        np.testing.assert_array_equal(new[0], ref[0])
        np.testing.assert_array_equal(new[1].view(np.uint32), ref[1].view(np.uint32))   # the same bits
        assert new[2] == ref[2]


@pytest.mark.parametrize("case", ["bench_like", "reference_init", "beta07", "k1_k256", "d32"])
def test_ondemand_route_equals_exact_and_split16_routes(case):
    from poi_recommendation_models_amd.synthetic import make_checkins
    P, U, hmax, D, H = 12000, 1500, 200, 64, 64
    kw = {}
    if case == "reference_init":
        kw = dict(emb_std=0.01)         # every score within ~1e-4 of 0.5: long survivor lists
    elif case == "beta07":
        kw = dict(beta=0.7)
    elif case == "d32":
        D, H = 32, 32
    data = make_checkins(U, P, hmax, seed=11)
    m = _model(P, D, H, **kw)
    for k in ((1, 256) if case == "k1_k256" else (50,)):
        _same_three(m, data, k)
    st = m._last_bound_stats.cpu().numpy()
    print(case, "refined per user", st[0] / U, "overflowed", st[1])


def test_ondemand_route_edge_users_and_column_shards():
    """Empty and one-item histories, a user with fewer candidates than k, a long history; column
    shards whose ends are not multiples of the 512-column block."""
    from poi_recommendation_models_amd.synthetic import make_checkins
    data = make_checkins(400, 3000, 120, seed=9)
    hist = [data.history(u) for u in range(data.num_users)]
    hist[3] = np.zeros(0, np.int64)
    hist[7] = np.zeros(0, np.int64)
    hist[9] = np.array([1234], np.int64)
    hist[10] = np.array([2999], np.int64)
    hist[11] = np.arange(0, 3000 - 30, dtype=np.int64)        # 30 candidates (k = 50 > 30)
    hist[12] = np.sort(np.random.default_rng(1).choice(3000, 1500, replace=False))
    data.indptr = np.concatenate([[0], np.cumsum([len(h) for h in hist])]).astype(np.int64)
    data.indices = np.concatenate(hist).astype(np.int64)
    m = _model(3000, 64, 64)
    users = np.array([u for u in range(data.num_users) if u != 11])
    _same_three(m, data, 50, users=users)
    _same_three(m, data, 50, cols=(0, 3000))       # user 11: column shards allow short lists
    for cols in ((0, 1500), (1234, 2801), (2801, 3000)):
        _same_three(m, data, 50, users=users, cols=cols)


def test_ondemand_route_overflow_refines_every_column():
    from poi_recommendation_models_amd import catalog
    from poi_recommendation_models_amd.synthetic import make_checkins
    data = make_checkins(200, 4000, 80, seed=17)
    m = _model(4000, 32, 32, emb_std=0.01)
    old = catalog.PAIR_SURV_CAP
    catalog.PAIR_SURV_CAP = 64
    try:
        new = _run(m, data, 60, "ondemand")
        st = m._last_bound_stats.cpu().numpy()
    finally:
        catalog.PAIR_SURV_CAP = old
    assert new[3] == ["ondemand"] and st[1] > 0, "no user overflowed"
    exact = _run(m, data, 60, "exact")
    np.testing.assert_array_equal(new[0], exact[0])
    np.testing.assert_array_equal(new[1].view(np.uint32), exact[1].view(np.uint32))
    assert new[2] == exact[2]


def test_eta_beyond_the_threshold_keeps_the_split16_route():
    """Saturating magnitudes: eta' > 2^-9, so the call stays on the split16 tables and says so."""
    from poi_recommendation_models_amd import catalog
    from poi_recommendation_models_amd.synthetic import make_checkins
    data = make_checkins(100, 2000, 40, seed=5)
    m = _model(2000, 32, 32, emb_std=3.0)
    assert catalog.ondemand_widening(m)[1] > catalog.PAIR_ONDEMAND_ETA_MAX
    assert _run(m, data, 50, "ondemand")[3] == ["split16"]


def _widening_bits(m):
    from poi_recommendation_models_amd import catalog
    w, eta, ds = catalog.ondemand_widening(m)
    return w.cpu().numpy().view(np.uint32).copy(), eta, ds


@pytest.mark.parametrize("writer", ["inplace", "load_state_dict", "adagrad", "trainer", "inplace_x8"])
def test_widening_cache_follows_every_writer(writer):
    """catalog.ondemand_widening caches (eta', delta_s) on the parameters' (data_ptr, version
    counter); a stale hit is a soundness matter (bounds that no longer cover the pairs can drop a
    winner), and the contract is that every writer bumps the counters -- the native optimizer and
    the in-tree trainer write through raw device pointers. After each writer the cached value must
    be the one a fresh computation gives, and the default route must still return the exact
    route's lists. `inplace_x8` takes eta' across the gate: the route changes to split16."""
    from poi_recommendation_models_amd import catalog, optim
    from poi_recommendation_models_amd.synthetic import make_checkins
    from test_gpu_train import _batch, _csr, _params, _trainer
    from test_gpu_train import _model as _train_model
    P, D, H = 1500, 64, 64
    data = make_checkins(150, P, 40, seed=8)
    m = _train_model(_params(P, D, H, seed=21)).eval()
    m.precision = "fp16x6"
    assert _run(m, data, 50, "ondemand")[3] == ["ondemand"]        # fills the cache
    assert "_widen_cache" in m.__dict__
    before = _widening_bits(m)
    hist, tgt, labels = _batch(P, 40, 4, seed=3)
    if writer in ("inplace", "inplace_x8"):
        with torch.no_grad():
            m.embed_history.weight.mul_(2)
            if writer == "inplace_x8":
                m.embed_history.weight.mul_(4)
                m.embed_target.weight.mul_(8)
    elif writer == "load_state_dict":
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        for k in ("embed_history.weight", "embed_target.weight"):
            sd[k] *= 2
        m.load_state_dict(sd)
    elif writer == "adagrad":
        m.train()
        o = optim.Adagrad(m.parameters(), lr=0.05)
        for q in m.parameters():
            q.grad = None
        pred = m(torch.as_tensor(hist).to(DEV), torch.as_tensor(tgt).to(DEV))
        m.loss_func(pred, torch.as_tensor(labels).to(DEV)).backward()
        o.step()
    else:
        m.train()
        tr = _trainer(m, _csr(3, P, 30, seed=4), lr=0.05)
        tr.step(torch.as_tensor(hist).to(DEV), torch.as_tensor(tgt).to(DEV), torch.as_tensor(labels).to(DEV))
        tr.finish()
    m.eval()
    torch.cuda.synchronize()
    # the default route first, on whatever the cache now answers
    new, exact = _run(m, data, 50, "ondemand"), _run(m, data, 50, "exact")
    np.testing.assert_array_equal(new[0], exact[0])
    np.testing.assert_array_equal(new[1].view(np.uint32), exact[1].view(np.uint32))
    assert new[2] == exact[2]
    cached = _widening_bits(m)
    m.__dict__.pop("_widen_cache", None)
    fresh = _widening_bits(m)
    print(writer, "eta' %.3e -> %.3e, delta_s %.3e -> %.3e, route %s" % (before[1], fresh[1], before[2], fresh[2], new[3]))
    assert cached[1] == fresh[1] and cached[2] == fresh[2]
    np.testing.assert_array_equal(cached[0], fresh[0])              # the device array, bit for bit
    assert (fresh[1], fresh[2]) != (before[1], before[2]) and not np.array_equal(fresh[0], before[0])
    if writer == "inplace_x8":
        assert fresh[1] > catalog.PAIR_ONDEMAND_ETA_MAX and new[3] == ["split16"], (fresh[1], new[3])


def _dist_setup():
    from poi_recommendation_models_amd.synthetic import make_checkins
    data = make_checkins(200, 2001, 80, seed=21)   # two column shards, 1001 and 1000 wide
    return data, _model(data.num_pois, 32, 32, seed=23)


def _dist_worker(rank, world, port, out):
    import torch.distributed as dist
    from poi_recommendation_models_amd import sharding
    from poi_recommendation_models_amd.catalog import DeviceCSR
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    data, m = _dist_setup()
    csr = DeviceCSR.from_arrays(data.indptr, data.indices, data.num_pois, DEV)
    ev = []
    ids, sc = sharding.distributed_topk_pairs(m, csr, np.arange(data.num_users), 50, events=ev)
    route = [v for kind, _, _, v in ev if kind == "pair_route"]
    np.savez(f"{out}_{rank}.npz", ids=ids.cpu().numpy(), sc=sc.cpu().numpy(), route=np.array(route))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_on_the_ondemand_route_equal_single_process():
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "r")
        mp.start_processes(_dist_worker, args=(2, port, out), nprocs=2, join=True, start_method="spawn")
        res = [np.load(f"{out}_{r}.npz") for r in range(2)]
    data, m = _dist_setup()
    ids, sc, _, route = _run(m, data, 50, "ondemand")
    assert route == ["ondemand"]
    for r in res:
        assert list(r["route"]) == ["ondemand"]
        np.testing.assert_array_equal(r["ids"], ids)
        np.testing.assert_array_equal(r["sc"].view(np.uint32), sc.view(np.uint32))
