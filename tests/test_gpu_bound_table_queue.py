"""GPU: the 3-product bound table as a work queue (include/nais.h nais_pair_table_bound_queued,
ABI 16; the x3b kernel's work loop).

1. Every word of the queued table equals the fixed-grid table's (nais_pair_table_bound, which is
   the same call with work = NULL) and the hi words of nais_pair_table_split at fp16x3 with
   work = NULL: across 128-row groups and a group tail, fewer items than workgroups, a partial
   last tile whose lanes clamp to row P - 1, on the default stream and on CU-masked streams of 40
   CUs (off the 32-CU shader-engine grid) and of 8 CUs (fewer CUs than work items, so a workgroup
   carries its state from item to item and from the first column tile into the second). The launch
   zeroes the counter itself, so the counter starts non-zero throughout.
2. The float (e, e*s) tables of nais_pair_table and the split16 (hi, ex) tables of
   nais_pair_table_split with a counter equal those without, every word: at fp16x3, and at fp16x6
   with embed_dim 16, which runs the same kernel with three pieces.
3. The on-demand job with the table stream on 168 and on 172 CUs (both streams then run as queues)
   returns the ids, score bits and NaN count of the job at 160 CUs and of the exact route."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
P_T, W_T = 3000, 512


def _model(P, D, H, seed=3, emb_std=0.3, spread=False):
    from poi_recommendation_models_amd import model as M
    from poi_recommendation_models_amd.synthetic import init_nais_params
    m = M.NAIS_basic(P, D, H, 0.5)
    p = init_nais_params(P, D, H, seed=seed, emb_std=emb_std, bias_std=0.1)
    if spread:   # per-row factors 1e-3 .. 1e2: chunks and tiles get different power-of-two scales
        rng = np.random.default_rng(seed + 100)
        for name in ("embed_history.weight", "embed_target.weight"):
            p[name] = (p[name] * 10.0 ** rng.uniform(-3, 2, (P, 1))).astype(np.float32)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()}, strict=False)
    m.precision = "fp16x6"
    m.report_nan = False
    return m.to(DEV).eval()


class _MaskedStream:
    """A stream on the first `cus` CUs (nais_stream_create_cu_mask); None = the default stream."""

    def __init__(self, cus):
        self.cus, self.handle = cus, None

    def __enter__(self):
        from poi_recommendation_models_amd import _capi
        if self.cus is None:
            return None
        n = torch.cuda.get_device_properties(DEV).multi_processor_count
        assert self.cus < n
        words = (n + 31) // 32
        mask = (ctypes.c_uint32 * words)()
        for c in range(self.cus):
            mask[c // 32] |= 1 << (c % 32)
        h = ctypes.c_void_p()
        _capi.check(_capi.load().nais_stream_create_cu_mask(mask, words, ctypes.byref(h)), "cu mask")
        self.handle = h.value
        return self.handle

    def __exit__(self, *exc):
        from poi_recommendation_models_amd import _capi
        if self.handle is not None:
            torch.cuda.synchronize()
            _capi.load().nais_stream_destroy(self.handle)
        return False


def _bound(m, items, c0, w, work, stream):
    from poi_recommendation_models_amd import _capi
    lib, J = _capi.load(), len(items)
    hi = torch.full((J, W_T), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()   # the fill (default stream) before a launch on another stream
    if work is None:
        rc = lib.nais_pair_table_bound(m._score_params(), items.data_ptr(), J, c0, w, None, None, None,
                                       hi.data_ptr(), W_T, stream)
    else:
        rc = lib.nais_pair_table_bound_queued(m._score_params(), items.data_ptr(), J, c0, w, None, None,
                                              None, hi.data_ptr(), W_T, work.data_ptr(), stream)
    _capi.check(rc, "nais_pair_table_bound")
    torch.cuda.synchronize()
    return hi.cpu().numpy().view(np.uint32)


def _split_hi(m, items, c0, w):
    from poi_recommendation_models_amd import _capi
    J = len(items)
    old, m.precision = m.precision, "fp16x3"
    try:
        hi = torch.zeros(J, W_T, dtype=torch.int32, device=DEV)
        ex = torch.zeros(J, 2 * W_T, dtype=torch.int32, device=DEV)
        _capi.check(_capi.load().nais_pair_table_split(m._score_params(), items.data_ptr(), J, c0, w, None,
                                                       None, None, hi.data_ptr(), ex.data_ptr(), W_T, None,
                                                       None), "nais_pair_table_split")
        torch.cuda.synchronize()
    finally:
        m.precision = old
    return hi.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("D,H", [(64, 64), (32, 32), (50, 40)])
def test_queued_bound_table_equals_the_fixed_grid_table(D, H):
    m = _model(P_T, D, H, emb_std=0.01, spread=True)
    cases = [(J, c0) for J in (300, 5, 700) for c0 in (0, 700, P_T - 200)]
    ref = {}
    for J, c0 in cases:   # the fixed grid (work = NULL), once per case, on the default stream
        items = torch.arange(5, 5 + J, dtype=torch.int64, device=DEV)
        w = min(W_T, P_T - c0)
        ref[J, c0] = _bound(m, items, c0, w, None, None)
        np.testing.assert_array_equal(ref[J, c0][:, :w], _split_hi(m, items, c0, w)[:, :w])
        assert np.all(ref[J, c0][:, w:] == 0x5A5A5A5A)   # nothing past the block
    work = torch.zeros(1, dtype=torch.int32, device=DEV)
    for cus in (None, 40, 8):
        with _MaskedStream(cus) as stream:
            for J, c0 in cases:
                items = torch.arange(5, 5 + J, dtype=torch.int64, device=DEV)
                w = min(W_T, P_T - c0)
                work.fill_(12345)   # the launch zeroes it, stream-ordered
                got = _bound(m, items, c0, w, work, stream)
                np.testing.assert_array_equal(got, ref[J, c0], err_msg=f"J={J} c0={c0} cus={cus}")
                ngroups, ntiles = (J + 127) // 128, (w + 255) // 256
                # it ran as a queue (D = 50 is padded to 64): every item taken, one miss per workgroup
                n = torch.cuda.get_device_properties(DEV).multi_processor_count
                wgs = min(ngroups * ntiles, n if cus is None else cus)
                assert int(work.item()) == ngroups * ntiles + wgs, (J, c0, cus, int(work.item()))


def _fp16x3_tables(m, items, c0, w, work, stream, precision="fp16x3"):
    """nais_pair_table's (e, e*s) and nais_pair_table_split's (hi, ex) at `precision`, as uint32 words."""
    from poi_recommendation_models_amd import _capi
    lib, J = _capi.load(), len(items)
    old, m.precision = m.precision, precision
    try:
        prm = m._score_params()
        f = torch.full((2, J, W_T), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        hi = torch.full((J, W_T), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        ex = torch.full((J, 2 * W_T), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        wp = None if work is None else work.data_ptr()
        _capi.check(lib.nais_pair_table(prm, items.data_ptr(), J, c0, w, None, None, None, f[0].data_ptr(),
                                        f[1].data_ptr(), W_T, wp, stream), "nais_pair_table")
        _capi.check(lib.nais_pair_table_split(prm, items.data_ptr(), J, c0, w, None, None, None,
                                              hi.data_ptr(), ex.data_ptr(), W_T, wp, stream),
                    "nais_pair_table_split")
        torch.cuda.synchronize()
    finally:
        m.precision = old
    return tuple(t.cpu().numpy().view(np.uint32) for t in (f, hi, ex))


@pytest.mark.parametrize("D,H,precision", [(64, 64, "fp16x3"), (32, 32, "fp16x3"),
                                           # fp16x6 at D = 16 runs the same kernel with three pieces
                                           # (per-wave scales in LDS): pipelined (H <= 64) and wide
                                           (16, 16, "fp16x6"), (16, 100, "fp16x6")])
def test_queued_fp16x3_float_and_split_tables_equal_the_fixed_grid(D, H, precision):
    """The same kernel behind nais_pair_table and nais_pair_table_split at fp16x3 (ABI 16: they take
    the counter too): the float (e, e*s) tables and the split16 (hi, ex) tables, every word, on the
    default stream and on 8 CUs (12 items of J = 700: state carried across items and tiles)."""
    m = _model(P_T, D, H, emb_std=0.01, spread=True)
    work = torch.zeros(1, dtype=torch.int32, device=DEV)
    cases = [(700, 0), (300, 700), (5, P_T - 200), (700, P_T - 200)]
    ref = {}
    for J, c0 in cases:
        items = torch.arange(5, 5 + J, dtype=torch.int64, device=DEV)
        ref[J, c0] = _fp16x3_tables(m, items, c0, min(W_T, P_T - c0), None, None, precision)
    for cus in (None, 8):
        with _MaskedStream(cus) as stream:
            for J, c0 in cases:
                items = torch.arange(5, 5 + J, dtype=torch.int64, device=DEV)
                work.fill_(777)
                got = _fp16x3_tables(m, items, c0, min(W_T, P_T - c0), work, stream, precision)
                ng, nt = (J + 127) // 128, (min(W_T, P_T - c0) + 255) // 256
                assert int(work.item()) > ng * nt   # it ran as a queue: every item and the misses
                for g, r, name in zip(got, ref[J, c0], ("e / e*s", "hi", "ex")):
                    np.testing.assert_array_equal(g, r, err_msg=f"{name} J={J} c0={c0} cus={cus}")


def _job(m, data, k, route, table_cus, cols=None):
    from poi_recommendation_models_amd import catalog
    from poi_recommendation_models_amd.catalog import DeviceCSR, _score_topk_pairs
    csr = DeviceCSR.from_arrays(data.indptr, data.indices, data.num_pois, DEV)
    old = catalog.PAIR_BOUNDED, catalog.PAIR_ONDEMAND_REFINE, catalog.PAIR_TABLE_CUS
    catalog.PAIR_BOUNDED, catalog.PAIR_ONDEMAND_REFINE = route != "exact", route == "ondemand"
    catalog.PAIR_TABLE_CUS = table_cus
    try:
        ev = []
        ids, sc = _score_topk_pairs(m, csr, np.arange(data.num_users), k, None, None, None, None, force=True,
                                    cols=cols, events=ev)
    finally:
        catalog.PAIR_BOUNDED, catalog.PAIR_ONDEMAND_REFINE, catalog.PAIR_TABLE_CUS = old
    torch.cuda.synchronize()
    took = [v for kind, _, _, v in ev if kind == "pair_route"]
    cus = [v for kind, _, _, v in ev if kind == "table_cus"]
    return ids.cpu().numpy(), sc.cpu().numpy(), int(m._last_nan.item()), took, cus


def test_ondemand_job_off_the_engine_grid_equals_160_and_exact():
    from poi_recommendation_models_amd.synthetic import make_checkins
    if torch.cuda.get_device_properties(DEV).multi_processor_count <= 172:
        pytest.fail("the splits under test (160, 168, 172 table CUs) need a device with more CUs")
    P, U, hmax, D, H, k = 12000, 1500, 200, 64, 64, 50
    data = make_checkins(U, P, hmax, seed=11)
    m = _model(P, D, H)
    for cols in (None, (3000, 9100)):
        exact = _job(m, data, k, "exact", -1, cols)
        at160 = _job(m, data, k, "ondemand", 160, cols)
        assert exact[3] == ["exact"] and at160[3] == ["ondemand"] and at160[4] == [160]
        for cus in (168, 172):
            got = _job(m, data, k, "ondemand", cus, cols)
            assert got[3] == ["ondemand"] and got[4] == [cus], (got[3], got[4])
            for ref in (at160, exact):
                np.testing.assert_array_equal(got[0], ref[0])
                np.testing.assert_array_equal(got[1].view(np.uint32), ref[1].view(np.uint32))
                assert got[2] == ref[2]
