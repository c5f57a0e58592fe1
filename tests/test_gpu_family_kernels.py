"""GPU: the C entry points behind the New4 family, called directly (through _capi.load(), as
test_gpu_topk.py does) and compared with float64 numpy restatements of include/nais.h's comments:
nais_near_attention, nais_copy_columns, nais_new4_tables (csrc/nais_new4.hip), nais_linear_rows,
nais_dot_forward, nais_dot_pair_table, nais_dot_single_fixup (csrc/nais_dot.hip).

The model-level tests (test_gpu_family.py, test_gpu_parity.py) reach these kernels at
embed_size = 32 and K <= 12 only; the reference driver runs the family at embed_size = hidden =
128 with 50 near POIs. The shapes here are the driver's and the ones where each kernel takes
another path: the second trip of the `lane += 64` loops (pool width or K above 64), launches
above 64 KiB of dynamic LDS, output widths that do not divide the workgroup, the grid-stride
loop, ragged tiles and slices of the pair table, column windows and chunk boundaries of the
one-item fixup.

Inputs: tables N(0, 0.3), Linear weights U(+-dim^-0.5), biases N(0, 0.1), fixed seeds; the
references read the same float32 bits in float64. Every test prints its largest error."""
import numpy as np
import pytest
import torch

from _helpers import SCORE_ATOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
SENT = 12345.0             # pre-fill of every output buffer: what a kernel must not touch keeps it
TABLE_ATOL = 1e-5          # the project's bound for these tables (test_family_tables_vs_oracle)
U24 = 2.0 ** -24           # float32 unit roundoff
E_INVALID, E_UNSUPPORTED = -1, -2


def _api():
    from poi_recommendation_models_amd import _capi
    return _capi, _capi.load(), _capi.stream_handle(torch.device(DEV))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _table(rng, *shape):
    return rng.normal(0, 0.3, shape).astype(F32)


def _linear(rng, dout, din, bias=True):
    w = rng.uniform(-din ** -0.5, din ** -0.5, (dout, din)).astype(F32)
    return w, (rng.normal(0, 0.1, dout).astype(F32) if bias else None)


def _sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def _near(rng, P, K):
    """Near-POI lists with repeated ids: one row all one POI, one row alternating, and (random
    draws with replacement) accidental repeats elsewhere."""
    near = rng.integers(0, P, (P, K)).astype(np.int64)
    near[5, :] = 7
    near[6, ::2] = near[6, 0]
    near[P - 1, :] = P - 1
    return near


# ------------------------------------------------------------------ nais_near_attention
def _ref_near(qsrc, kvsrc, near, scale_dim, lin=None):
    """include/nais.h: x_k = kv[near[p][k]], q = query[near[p][0]], optional nn.Linear on q, keys,
    values; out = softmax(q . reshape(key, [dim, K]) / sqrt(scale_dim)) @ val -- the [K, dim] keys
    REINTERPRETED as [dim, K] (reshape, not transpose). float64."""
    x = kvsrc.astype(F64)[near]                                  # [P, K, d]
    P, K, d = x.shape
    q = qsrc.astype(F64)[near[:, 0]]
    keys = vals = x
    if lin is not None:
        wq, bq, wk, bk, wv, bv = (a.astype(F64) for a in lin)
        q, keys, vals = q @ wq.T + bq, x @ wk.T + bk, x @ wv.T + bv
    keys = np.ascontiguousarray(keys).reshape(P, d, K)
    lg = np.einsum("pa,pab->pb", q, keys) / np.sqrt(F64(scale_dim))
    w = np.exp(lg - lg.max(-1, keepdims=True))
    w /= w.sum(-1, keepdims=True)
    return np.einsum("pb,pbc->pc", w, vals)


# (pool width d, near POIs K): the shape tested elsewhere as a control; the driver's; the second
# trip of the `lane += 64` loops on d with a single-element softmax; on d and on K; 124,224 bytes
# of dynamic LDS (above the 64 KiB a launch gets without hipFuncSetAttribute)
NEAR_SHAPES = [(8, 10), (32, 50), (64, 50), (65, 1), (100, 65), (128, 80)]


@pytest.mark.parametrize("projected", [False, True], ids=["plain", "projected"])
@pytest.mark.parametrize("d,K", NEAR_SHAPES)
def test_near_attention_vs_float64(d, K, projected):
    _capi, lib, st = _api()
    rng = np.random.default_rng(1000 * d + 2 * K + projected)
    P, c0, ld = 211, 3, d + 7
    qsrc, kvsrc, near = _table(rng, P, d), _table(rng, P, d), _near(rng, P, K)
    lin = None
    if projected:
        lin = [a for _ in range(3) for a in _linear(rng, d, d)]
    tq, tkv, tn = _dev(qsrc), _dev(kvsrc), _dev(near)
    tl = [None] * 6 if lin is None else [_dev(a) for a in lin]
    tab = torch.full((P, ld), SENT, dtype=torch.float32, device=DEV)
    _capi.check(lib.nais_near_attention(tq.data_ptr(), tkv.data_ptr(), P, d, tn.data_ptr(), K,
                                        *[_capi.ptr(a) for a in tl], float(d),
                                        tab.data_ptr() + 4 * c0, ld, st), "nais_near_attention")
    got = tab.cpu().numpy()
    ref = _ref_near(qsrc, kvsrc, near, d, lin)
    assert np.all(got[:, :c0] == F32(SENT)) and np.all(got[:, c0 + d:] == F32(SENT))
    err = float(np.max(np.abs(got[:, c0:c0 + d] - ref)))
    print(f"near_attention d={d} K={K} projected={projected}: max |err| {err:.3g} (bound {TABLE_ATOL})")
    assert err <= TABLE_ATOL


# ------------------------------------------------------------------ nais_copy_columns
def test_copy_columns_bit_exact():
    _capi, lib, st = _api()
    rng = np.random.default_rng(31)
    rows, dim, src_ld, dst_ld, col0 = 301, 37, 41, 50, 9
    src = _table(rng, rows, src_ld)
    src[0, 0], src[1, 1], src[2, 2] = np.nan, np.inf, -0.0        # bit patterns, not values
    ts = _dev(src)
    dst = torch.full((rows, dst_ld), SENT, dtype=torch.float32, device=DEV)
    _capi.check(lib.nais_copy_columns(ts.data_ptr(), src_ld, rows, dim, dst.data_ptr(), dst_ld, col0, st),
                "nais_copy_columns")
    want = np.full((rows, dst_ld), SENT, F32)
    want[:, col0:col0 + dim] = src[:, :dim]
    np.testing.assert_array_equal(dst.cpu().numpy().view(np.int32), want.view(np.int32))
    # rows = 0: accepted, nothing written
    dst.fill_(SENT)
    assert lib.nais_copy_columns(ts.data_ptr(), src_ld, 0, dim, dst.data_ptr(), dst_ld, col0, st) == 0
    assert bool((dst == SENT).all())
    # a column range that does not fit the destination rows is refused, nothing written
    assert lib.nais_copy_columns(ts.data_ptr(), src_ld, rows, dim, dst.data_ptr(), dst_ld,
                                 dst_ld - dim + 1, st) == E_INVALID
    assert bool((dst == SENT).all())


# ------------------------------------------------------------------ nais_new4_tables
@pytest.mark.parametrize("K", [1, 50])
@pytest.mark.parametrize("E", [12, 48, 128, 256])
def test_new4_tables_vs_float64(E, K):
    """ext_history = [embed_history | in | out], ext_target = [embed_target | out | in] with
    in = pool of embed_ingoing queried by embed_outgoing, out the reverse, scale_dim = E / 4."""
    _capi, lib, st = _api()
    rng = np.random.default_rng(7 * E + K)
    P, half, d4 = 203, E // 2, E // 4
    eh, et = _table(rng, P, half), _table(rng, P, half)
    ein, eout = _table(rng, P, d4), _table(rng, P, d4)
    near = _near(rng, P, K)
    dev = [_dev(a) for a in (eh, et, ein, eout)]
    tn = _dev(near)
    xh = torch.full((P, E), SENT, dtype=torch.float32, device=DEV)
    xt = torch.full((P, E), SENT, dtype=torch.float32, device=DEV)
    _capi.check(lib.nais_new4_tables(*[a.data_ptr() for a in dev], P, E, tn.data_ptr(), K,
                                     xh.data_ptr(), xt.data_ptr(), st), "nais_new4_tables")
    xh, xt = xh.cpu().numpy(), xt.cpu().numpy()
    np.testing.assert_array_equal(xh[:, :half].view(np.int32), eh.view(np.int32))
    np.testing.assert_array_equal(xt[:, :half].view(np.int32), et.view(np.int32))
    r_in = _ref_near(eout, ein, near, E / 4)
    r_out = _ref_near(ein, eout, near, E / 4)
    err = max(float(np.max(np.abs(xh[:, half:half + d4] - r_in))),
              float(np.max(np.abs(xh[:, half + d4:] - r_out))))
    print(f"new4_tables E={E} K={K}: max |pool err| {err:.3g} (bound {TABLE_ATOL})")
    assert err <= TABLE_ATOL
    np.testing.assert_array_equal(xt[:, half:half + d4].view(np.int32), xh[:, half + d4:].view(np.int32))
    np.testing.assert_array_equal(xt[:, half + d4:].view(np.int32), xh[:, half:half + d4].view(np.int32))


# ------------------------------------------------------------------ nais_linear_rows
def _run_linear(rng, rows, din, dout, bias):
    _capi, lib, st = _api()
    x_ld, y_ld = din + 5, dout + 3
    x = _table(rng, rows, x_ld)
    w, b = _linear(rng, dout, din, bias)
    tx, tw, tb = _dev(x), _dev(w), (_dev(b) if bias else None)
    y = torch.full((rows, y_ld), SENT, dtype=torch.float32, device=DEV)
    _capi.check(lib.nais_linear_rows(tx.data_ptr(), x_ld, rows, din, tw.data_ptr(), _capi.ptr(tb), dout,
                                     y.data_ptr(), y_ld, st), "nais_linear_rows")
    got = y.cpu().numpy()
    ref = x[:, :din].astype(F64) @ w.astype(F64).T + (b.astype(F64) if bias else 0.0)
    assert np.all(got[:, dout:] == F32(SENT))
    return float(np.max(np.abs(got[:, :dout] - ref)))


# (1, 1): 256 rows per workgroup. (48, 48): 5 rows per workgroup, 16 idle threads that return
# after the barrier. (100, 200) and (200, 200): one row per workgroup, 56 idle threads, 80,000 and
# 160,000 bytes of dynamic LDS (above 64 KiB: needs the hipFuncSetAttribute call). (128, 128):
# transform_attn's projections at the driver's width, exactly 64 KiB.
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("din,dout", [(1, 1), (48, 48), (100, 200), (128, 128), (200, 200)])
def test_linear_rows_vs_float64(din, dout, bias):
    err = _run_linear(np.random.default_rng(din * 1000 + dout + bias), 257, din, dout, bias)
    print(f"linear_rows {din}->{dout} bias={bias}: max |err| {err:.3g} (bound {TABLE_ATOL})")
    assert err <= TABLE_ATOL


def test_linear_rows_grid_stride():
    """rows = 9000 at dout = 200: one row per workgroup and a grid capped at 8192 workgroups, so
    the first 808 workgroups take a second row."""
    err = _run_linear(np.random.default_rng(9000), 9000, 100, 200, True)
    print(f"linear_rows 100->200 rows=9000: max |err| {err:.3g} (bound {TABLE_ATOL})")
    assert err <= TABLE_ATOL


# ------------------------------------------------------------------ the dot core's tables
class _Dot:
    """Five [P, D] float32 tables (built on the host, so the device and the float64 references
    read the same bits) and their nais_dot_tables_t; scale_dim = D as transform_attn sets it."""

    def __init__(self, rng, P, D):
        from poi_recommendation_models_amd import _capi
        self.P, self.D = P, D
        self.np = {n: _table(rng, P, D) for n in ("xh", "xt", "qt", "kh", "vh")}
        self.dev = {n: _dev(a) for n, a in self.np.items()}
        self.f64 = {n: a.astype(F64) for n, a in self.np.items()}
        self.scale = np.sqrt(F64(D))
        t = _capi.NaisDotTables()
        t.embed_dim, t.num_pois, t.beta, t.scale_dim = D, P, 0.5, float(D)
        for n, a in self.dev.items():
            setattr(t, n, a.data_ptr())
        self.c = t

    def logits(self, hist, target):
        """nais_dot_forward's logits in float64. n >= 2 (or 0): sum_j m_j e_j s_j / (sum_j m_j
        e_j)^0.5, m_j = [h_j != c], 0 for an empty history. n == 1: every row pools exp over ALL
        rows of the call, out_r = m_r s_r S / (m_r S)^0.5 (0/0 = NaN when masked)."""
        b, n = hist.shape
        if n == 0:
            return np.zeros(b)
        k, v = self.f64["kh"][hist], self.f64["vh"][hist]               # [b, n, D]
        q, x = self.f64["qt"][target][:, None, :], self.f64["xt"][target][:, None, :]
        e = np.exp((q * k).sum(-1) / self.scale)
        s = (v * x).sum(-1)
        m = hist != target[:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            if n == 1:
                S = e.sum()
                return np.where(m[:, 0], s[:, 0] * S / np.sqrt(S), np.nan)
            e = e * m
            return (e * s).sum(-1) / np.sqrt(e.sum(-1))

    def forward(self, hist, target, flags, hist_ld_extra=3):
        """nais_dot_forward on a strided history (row pitch n + hist_ld_extra)."""
        _capi, lib, st = _api()
        b, n = hist.shape
        wide = np.full((b, n + hist_ld_extra), -1, np.int64)           # -1: never read
        wide[:, 1:1 + n] = hist
        th, tt = _dev(wide), _dev(target)
        out = torch.full((b,), SENT, dtype=torch.float32, device=DEV)
        nan = torch.zeros(1, dtype=torch.int32, device=DEV)
        _capi.check(lib.nais_dot_forward(self.c, th.data_ptr() + 8 if n else None, b, n,
                                         n + hist_ld_extra if n else 0, tt.data_ptr(), out.data_ptr(),
                                         nan.data_ptr(), flags, st), "nais_dot_forward")
        return out.cpu().numpy(), int(nan.item())


def _check_forward(t, hist, target, tag):
    ref = t.logits(hist, target)
    for flags, want in ((0, ref), (1, _sigmoid(ref))):
        got, nan = t.forward(hist, target, flags)
        assert np.array_equal(np.isnan(got), np.isnan(want)), tag
        assert nan == int(np.isnan(want).sum()), tag
        ok = ~np.isnan(want)
        err = float(np.max(np.abs(got[ok] - want[ok]))) if ok.any() else 0.0
        print(f"dot_forward {tag} {'scores' if flags else 'logits'}: max |err| {err:.3g} "
              f"(bound {SCORE_ATOL}), max |ref| {float(np.max(np.abs(want[ok]))) if ok.any() else 0:.3g}")
        assert err <= SCORE_ATOL, tag
    return ref


# D = 1; an odd width; exactly one element per lane; the `lane + 64 < D` half with 1 and 32 live
# lanes; two full elements per lane
@pytest.mark.parametrize("n", [0, 2, 37])
@pytest.mark.parametrize("D", [1, 33, 64, 65, 96, 128])
def test_dot_forward_vs_float64(D, n):
    rng = np.random.default_rng(100 * D + n)
    P, b = 257, 41
    t = _Dot(rng, P, D)
    hist = rng.integers(0, P, (b, n)).astype(np.int64)
    target = rng.integers(0, P, b).astype(np.int64)
    if n:
        target[2], target[9] = hist[2, 0], hist[9, n - 1]      # one masked item
        hist[17, :] = target[17]                               # every item masked: 0 / 0
    ref = _check_forward(t, hist, target, f"D={D} n={n}")
    if n:
        assert np.isnan(ref[17]) and not np.isnan(ref[[2, 9]]).any()
    else:
        assert np.all(ref == 0.0)


@pytest.mark.parametrize("b", [5, 1500])
def test_dot_forward_one_item_batches(b):
    """n == 1 at D = 96: the batch-coupled kernel, within one pass of its 1024 threads and past it."""
    rng = np.random.default_rng(b)
    P = 257
    t = _Dot(rng, P, 96)
    hist = rng.integers(0, P, (b, 1)).astype(np.int64)
    target = rng.integers(0, P, b).astype(np.int64)
    target[hist[:, 0] == target] = (target[hist[:, 0] == target] + 1) % P
    target[1::4] = hist[1::4, 0]                               # masked rows: NaN
    ref = _check_forward(t, hist, target, f"D=96 n=1 b={b}")
    assert int(np.isnan(ref).sum()) == len(range(1, b, 4))


def test_dot_forward_width_above_128_is_unsupported():
    _capi, lib, st = _api()
    t = _Dot(np.random.default_rng(129), 50, 129)
    tt = _dev(np.zeros(4, np.int64))
    th = _dev(np.zeros((4, 2), np.int64))
    out = torch.full((4,), SENT, dtype=torch.float32, device=DEV)
    assert lib.nais_dot_forward(t.c, th.data_ptr(), 4, 2, 2, tt.data_ptr(), out.data_ptr(), None, 1,
                                st) == E_UNSUPPORTED
    assert bool((out == SENT).all())


# ------------------------------------------------------------------ nais_dot_pair_table
def _pair_table(t, items, col0, cols, ld):
    _capi, lib, st = _api()
    J = len(items)
    ti = _dev(items)
    e = torch.full((J, ld), SENT, dtype=torch.float32, device=DEV)
    es = torch.full((J, ld), SENT, dtype=torch.float32, device=DEV)
    _capi.check(lib.nais_dot_pair_table(t.c, ti.data_ptr(), J, col0, cols, e.data_ptr(), es.data_ptr(),
                                        ld, st), "nais_dot_pair_table")
    return e, es


# D: one ragged 32-wide slice; exactly one; two with a ragged last; three; four.
# J: one item; a ragged 64-row tile; three row tiles with a ragged last.
@pytest.mark.parametrize("J", [1, 63, 130])
@pytest.mark.parametrize("D", [20, 32, 33, 96, 128])
def test_dot_pair_table_vs_float64(D, J):
    """E[j, c] = exp(qt_c . kh_j / sqrt(D)), ES = E * (vh_j . xt_c) over column windows -- full
    rows, a window inside them (col0 > 0, ragged column tiles) and the last five columns -- into
    tables three columns wider than the window.

    Tolerance, per element, from the float64 operands (u = 2^-24): a length-D fp32 fma chain is
    within D u sum|q_i k_i| of the dot, so |de| <= e (D u sum|q_i k_i| / scale + 4 u), the 4 u for
    expf and the division; |ds| <= D u sum|v_i x_i|; |d(e s)| <= |de| |s| + e |ds| + |de| |ds| +
    u |e s| (one rounding of the product); both doubled for the device expf."""
    _capi, lib, st = _api()
    rng = np.random.default_rng(1000 * D + J)
    P = 230
    t = _Dot(rng, P, D)
    items = np.sort(rng.choice(P, J, replace=False)).astype(np.int64)
    k, v = t.f64["kh"][items], t.f64["vh"][items]
    worst = 0.0
    for col0, cols in ((0, P), (37, 70), (P - 5, 5)):
        ld = cols + 3
        e, es = _pair_table(t, items, col0, cols, ld)
        e, es = e.cpu().numpy(), es.cpu().numpy()
        assert np.all(e[:, cols:] == F32(SENT)) and np.all(es[:, cols:] == F32(SENT))
        q, x = t.f64["qt"][col0:col0 + cols], t.f64["xt"][col0:col0 + cols]
        re = np.exp(k @ q.T / t.scale)
        rs = v @ x.T
        be = re * (D * U24 * (np.abs(k) @ np.abs(q).T) / t.scale + 4 * U24)
        bs = D * U24 * (np.abs(v) @ np.abs(x).T)
        bes = be * np.abs(rs) + re * bs + be * bs + U24 * np.abs(re * rs)
        de, des = np.abs(e[:, :cols] - re), np.abs(es[:, :cols] - re * rs)
        worst = max(worst, float(np.max(de / (2 * be))), float(np.max(des / (2 * bes))))
        assert np.all(de <= 2 * be), (col0, cols, float(np.max(de / (2 * be))))
        assert np.all(des <= 2 * bes), (col0, cols, float(np.max(des / (2 * bes))))
    print(f"dot_pair_table D={D} J={J}: largest error / bound {worst:.3g} "
          f"(bounds: median {float(np.median(2 * be)):.3g} on e, {float(np.median(2 * bes)):.3g} on es)")

    # the two routes tied together: these tables through nais_pair_gather against
    # nais_dot_forward on the same (history, candidate) rows
    col0, cols = 37, 70
    ld = (cols + 3) // 4 * 4                                   # the gather reads 4 columns at a time
    e, es = _pair_table(t, items, col0, cols, ld)
    n = min(J, 5)
    U = 3
    hists = [rng.choice(J, n, replace=False) for _ in range(U)]          # rows of items[]
    rowmap = np.full(P, -1, np.int32)
    rowmap[items] = np.arange(J, dtype=np.int32)
    indptr = np.arange(U + 1, dtype=np.int64) * n
    indices = np.concatenate([items[h] for h in hists]).astype(np.int64)
    dev = [_dev(a) for a in (rowmap, indptr, indices, np.arange(U, dtype=np.int32))]
    scores = torch.full((U, cols), SENT, dtype=torch.float32, device=DEV)
    nan = torch.zeros(1, dtype=torch.int32, device=DEV)
    _capi.check(lib.nais_pair_gather(e.data_ptr(), es.data_ptr(), ld, *[a.data_ptr() for a in dev], U,
                                     col0, cols, 0.5, scores.data_ptr(), cols, col0, nan.data_ptr(), st),
                "nais_pair_gather")
    scores = scores.cpu().numpy()
    assert int(nan.item()) == 0
    tie = 0.0
    for u in range(U):
        hist = items[hists[u]]
        cand = np.setdiff1d(np.arange(col0, col0 + cols), hist)
        assert np.all(scores[u][np.intersect1d(hist, np.arange(col0, col0 + cols)) - col0] == -1.0)
        if n == 1:
            # a one-item forward couples the rows of its call; alone in it (b = 1) a row is the
            # gather's sigmoid(e s / e^0.5)
            cand = cand[[0, len(cand) // 2, -1]]
            fwd = np.array([t.forward(hist[None, :], cand[i:i + 1], 1)[0][0] for i in range(len(cand))])
        else:
            fwd = t.forward(np.broadcast_to(hist, (len(cand), n)), cand, 1)[0]
        tie = max(tie, float(np.max(np.abs(scores[u][cand - col0] - fwd))))
    print(f"dot_pair_table D={D} J={J}: gather vs forward max |diff| {tie:.3g} (bound {SCORE_ATOL})")
    assert tie <= SCORE_ATOL


# ------------------------------------------------------------------ nais_dot_single_fixup
def test_dot_single_fixup_vs_float64():
    """P = 2500 (three 1024-candidate chunks of the complement list, the last one ragged:
    P - 1 = 2499), D = 96. One-item users with the history POI first, on both sides of a chunk
    boundary (c = i + (i >= h): h = 1023 is the last candidate slot of chunk 0, h = 1024 the
    first of chunk 1) and last; two longer histories the call must leave alone. Column windows as
    a column shard passes them (score_col0 = col0, score_ld = cols): full rows, one inside chunk
    0, one that starts 8 columns before chunk 2 and runs to P -- S_k is still summed over the
    whole chunk."""
    _capi, lib, st = _api()
    rng = np.random.default_rng(2500)
    P, D = 2500, 96
    t = _Dot(rng, P, D)
    singles = [0, 1023, 1024, P - 1]
    hists = [[h] for h in singles] + [[5, 1500], list(range(100, 2400, 300))]
    indptr = np.cumsum([0] + [len(h) for h in hists]).astype(np.int64)
    indices = np.concatenate(hists).astype(np.int64)
    U = len(hists)
    dev = [_dev(a) for a in (indptr, indices, np.arange(U, dtype=np.int32))]
    ref = np.full((U, P), SENT)
    for u, h in enumerate(singles):
        cand = np.setdiff1d(np.arange(P), [h])
        e = np.exp(t.f64["qt"][cand] @ t.f64["kh"][h] / t.scale)
        s = t.f64["xt"][cand] @ t.f64["vh"][h]
        for a in range(0, P - 1, 1024):
            S = e[a:a + 1024].sum()
            ref[u, cand[a:a + 1024]] = _sigmoid(s[a:a + 1024] * S / np.sqrt(S))
    worst = 0.0
    for col0, cols in ((0, P), (1000, 100), (2040, 460)):
        scores = torch.full((U, cols), SENT, dtype=torch.float32, device=DEV)
        _capi.check(lib.nais_dot_single_fixup(t.c, *[a.data_ptr() for a in dev], U, col0, cols,
                                              scores.data_ptr(), cols, col0, st), "nais_dot_single_fixup")
        got = scores.cpu().numpy().astype(F64)
        want = ref[:, col0:col0 + cols]
        keep = want == SENT                    # the c = h slots and the longer-history users' rows
        assert keep[len(singles):].all() and keep[:len(singles)].sum() == \
            sum(col0 <= h < col0 + cols for h in singles)
        assert np.all(got[keep] == SENT), (col0, cols)
        err = float(np.max(np.abs(got[~keep] - want[~keep])))
        worst = max(worst, err)
        assert err <= SCORE_ATOL, (col0, cols, err)
    print(f"dot_single_fixup: max |err| {worst:.3g} (bound {SCORE_ATOL})")
