"""The three device-side batch builders (nais_make_train_batch, nais_bpr_make_train_batch,
nais_geoie_make_train_batch) held to the exact batch of the host model tests/_sampler_ref.py,
position by position, at history lengths where the block-wide candidate loop takes a second and a
third pass (BATCH_THREADS = 1024 candidates per pass for NAIS / GeoIE, BB_THREADS = 256 for BPR)
and where geoie_batch_fill_kernel has a second column tile. The distribution of the model's
batches is tests/test_sampler_ref.py's business; this file only shows that the kernels compute the
model.

Every comparison starts from outputs that hold a sentinel (-7 for ids, NaN for floats): the C entry
points are called on fresh prefilled buffers, and the trainers' own buffers, which they reuse for
calls of one shape, are prefilled between calls. A position the kernel never wrote cannot pass,
and the fresh buffers carry a few sentinel elements behind their end that must survive."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _geoie_oracle as go
import _sampler_ref as sr
from test_gpu_geoie_train import make_model as geoie_model
from test_gpu_geoie_train import shape_case
from poi_recommendation_models_amd import _capi
from poi_recommendation_models_amd.catalog import device_csr
from poi_recommendation_models_amd.model import BPR, NAIS_basic
from poi_recommendation_models_amd.trainer import BPRTrainer, GeoIETrainer, NAISTrainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEEDS = (7, 0xFFFFFFFF, (0x9E3779B9 << 32) | 12345)       # hi == 0, lo all ones, hi != 0
ID_SENTINEL = -7


def _poison(*tensors):
    for t in tensors:
        t.fill_(float("nan") if t.is_floating_point() else ID_SENTINEL)


GUARD = 8


def _fresh(n, dtype):
    """n sentinel-filled elements, the view of a buffer with GUARD more behind them: _guard_intact
    then shows that nothing was written past the end (a `pos <= want` cut writes one row too many)."""
    t = torch.empty(n + GUARD, dtype=dtype, device=DEV)
    _poison(t)
    return t[:n]


def _guard_intact(*views):
    for v in views:
        tail = v._base[v.numel():]
        assert tail.numel() == GUARD
        if not bool((torch.isnan(tail) if v.is_floating_point() else tail == ID_SENTINEL).all()):
            return False
    return True


def _csr(rows, P):
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.concatenate([np.asarray(r, np.int64) for r in rows] + [np.zeros(0, np.int64)])
    return sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(len(rows), P))


def _rows(lens, P, seed):
    rng = np.random.default_rng(seed)
    return [np.sort(rng.choice(P, h, replace=False)) for h in lens]


def _np(ts):
    return [t.cpu().numpy() for t in ts]


# --------------------------------------------------------------------------------------- NAIS
def _nais_direct(X, uid, n, ng, seed):
    """nais_make_train_batch on fresh sentinel-filled outputs: (hist, target, labels, err)."""
    csr = device_csr(X, DEV)
    b = n * (1 + ng)
    hist, tgt = _fresh(n, torch.int64), _fresh(b, torch.int64)
    lab, err = _fresh(b, torch.float32), torch.zeros(1, dtype=torch.int32, device=DEV)
    try:
        _capi.check(_capi.load().nais_make_train_batch(
            csr.indptr.data_ptr(), csr.indices.data_ptr(), int(uid), n, csr.shape[1], ng, seed,
            hist.data_ptr(), tgt.data_ptr(), lab.data_ptr(), err.data_ptr(), _capi.stream_handle(torch.device(DEV))),
            "nais_make_train_batch")
    finally:
        torch.cuda.synchronize()
    assert _guard_intact(hist, tgt, lab), "a write past the end of an output"
    return _np((hist, tgt, lab, err))


def _assert_nais(got, want, what):
    for g, w, name in zip(got, want, ("hist", "target", "labels")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name)


_NAIS_LENS = (1, 2, 204, 205, 300, 410)


@pytest.fixture(scope="module")
def nais3000():
    rows = _rows(_NAIS_LENS, 3000, 11)
    X = _csr(rows, 3000)
    return rows, X, NAISTrainer(NAIS_basic(3000, 8, 8, 0.5).to(DEV), X, num_ng=4)


# h (ng + 1) candidates in passes of 1024: 204 -> 1020, the last single pass; 205 -> 1025, a second
# pass with one live lane; 300 -> a full second pass; 410 -> 2050, a third pass with two live lanes
@pytest.mark.parametrize("h", _NAIS_LENS)
def test_nais_batch_equals_model(nais3000, h):
    rows, X, tr = nais3000
    u = _NAIS_LENS.index(h)
    for seed in SEEDS:
        want = sr.nais_batch(rows[u], 3000, 4, seed)
        got = _nais_direct(X, u, h, 4, seed)
        _assert_nais(got, want, (h, seed, "C entry point"))
        assert got[3][0] == 0
        bufs = tr.batch(u, seed=seed)
        _assert_nais(_np(bufs), want, (h, seed, "NAISTrainer.batch"))
        _poison(*bufs)          # the trainer hands the same buffers to the next call of this shape
    assert tr.finish() == 0.0


def test_nais_batch_uses_every_poi():
    """n (ng + 1) == P: all P candidates are drawn and all n ng non-positives are taken, so the
    negatives are the whole complement -- in the model's order."""
    P, h, ng = 1500, 300, 4
    rows = _rows([3, h], P, 12)
    X = _csr(rows, P)
    tr = NAISTrainer(NAIS_basic(P, 8, 8, 0.5).to(DEV), X, num_ng=ng)
    free = np.setdiff1d(np.arange(P), rows[1])
    for seed in SEEDS:
        want = sr.nais_batch(rows[1], P, ng, seed)
        for got in (_nais_direct(X, 1, h, ng, seed), _np(tr.batch(1, seed=seed))):
            _assert_nais(got, want, seed)
            neg = got[1].reshape(h, 1 + ng)[:, 1:].reshape(-1)
            assert np.array_equal(np.sort(neg), free)
    assert tr.finish() == 0.0


def test_nais_batch_single_poi_no_negatives():
    """P = 1, ng = 0: mn == mP == 1, the permutation is the constant 0 and the one candidate is
    the positive; the batch is that positive alone."""
    X = _csr([[0]], 1)
    tr = NAISTrainer(NAIS_basic(1, 8, 8, 0.5).to(DEV), X, num_ng=0)
    for seed in SEEDS:
        want = sr.nais_batch([0], 1, 0, seed)
        assert want[1].tolist() == [0] and want[2].tolist() == [1.0]
        _assert_nais(_nais_direct(X, 0, 1, 0, seed), want, seed)
        bufs = tr.batch(0, seed=seed)
        _assert_nais(_np(bufs), want, seed)
        _poison(*bufs)
    assert tr.finish() == 0.0


def test_nais_batch_one_row_too_many_is_refused():
    """n (ng + 1) == P + 1: NaisError before any launch -- the outputs keep their sentinels."""
    P, h, ng = 1499, 300, 4
    rows = _rows([h], P, 13)
    X = _csr(rows, P)
    csr = device_csr(X, DEV)
    hist, tgt, lab = _fresh(h, torch.int64), _fresh(h * 5, torch.int64), _fresh(h * 5, torch.float32)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(_capi.NaisError):
        _capi.check(_capi.load().nais_make_train_batch(
            csr.indptr.data_ptr(), csr.indices.data_ptr(), 0, h, P, ng, 5, hist.data_ptr(), tgt.data_ptr(),
            lab.data_ptr(), err.data_ptr(), _capi.stream_handle(torch.device(DEV))), "nais_make_train_batch")
    torch.cuda.synchronize()
    assert bool((hist == ID_SENTINEL).all()) and bool((tgt == ID_SENTINEL).all())
    assert bool(torch.isnan(lab).all()) and int(err.item()) == 0
    tr = NAISTrainer(NAIS_basic(P, 8, 8, 0.5).to(DEV), X, num_ng=ng)
    with pytest.raises(_capi.NaisError):
        tr.batch(0, seed=5)


# ---------------------------------------------------------------------------------------- BPR
def _bpr_direct(X, users, seed):
    """nais_bpr_make_train_batch on fresh sentinel-filled outputs: (user, item_i, item_j, err)."""
    csr = device_csr(X, DEV)
    users = np.asarray(users, np.int64)
    hl = csr.hist_len[users]
    off = np.concatenate([[0], np.cumsum(hl)[:-1]]).astype(np.int64)
    n = int(hl.sum())
    u, i, j = (_fresh(n, torch.int64) for _ in range(3))
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ud, od = torch.from_numpy(users).to(DEV), torch.from_numpy(off).to(DEV)
    _capi.check(_capi.load().nais_bpr_make_train_batch(
        csr.indptr.data_ptr(), csr.indices.data_ptr(), csr.shape[0], ud.data_ptr(), od.data_ptr(),
        len(users), csr.shape[1], seed, u.data_ptr(), i.data_ptr(), j.data_ptr(), err.data_ptr(),
        _capi.stream_handle(torch.device(DEV))), "nais_bpr_make_train_batch")
    torch.cuda.synchronize()
    assert _guard_intact(u, i, j), "a write past the end of an output"
    return _np((u, i, j, err))


def _bpr_want(rows, users, P, seed):
    parts = [sr.bpr_batch(rows[u], u, P, seed) for u in users]
    return [np.concatenate([p[c] for p in parts]) for c in range(3)]


def test_bpr_batch_equals_model():
    """2 h candidates per user in passes of 256: h = 128 is the last single pass, 129 a second
    pass with two live lanes, 300 a third, 600 = P / 2 a fifth in which every POI outside the
    history is taken. The users are listed unsorted, the empty one in the middle.

    User 6 is listed twice and gets the same negatives both times: the per-user seed depends only
    on (seed, u). That is the kernel's documented construction (one seed per user) and harmless
    inside an epoch, whose users are distinct."""
    P = 1200
    lens = [129, 0, 600, 1, 300, 64, 128]
    rows = _rows(lens, P, 21)
    X = _csr(rows, P)
    users = [2, 6, 3, 1, 4, 6, 0, 5]
    tr = BPRTrainer(BPR(len(lens), P, 4).to(DEV), X)
    for seed in SEEDS:
        want = _bpr_want(rows, users, P, seed)
        assert len(want[0]) == sum(lens[u] for u in users)
        got = _bpr_direct(X, users, seed)
        for g, w, name in zip(got, want, ("user", "item_i", "item_j")):
            assert np.array_equal(g, w), (seed, name, "C entry point")
        assert got[3][0] == 0
        for g, w, name in zip(_np(tr.batch(users, seed=seed)), want, ("user", "item_i", "item_j")):
            assert g.dtype == np.int64 and np.array_equal(g, w), (seed, name, "BPRTrainer.batch")
        j = got[2]
        o = np.concatenate([[0], np.cumsum([lens[u] for u in users])])
        assert np.array_equal(j[o[1]:o[2]], j[o[5]:o[6]])                  # user 6, both listings
        assert np.array_equal(np.sort(j[o[0]:o[1]]), np.setdiff1d(np.arange(P), rows[2]))   # h = P / 2
    assert tr.finish() == 0.0


def test_bpr_batch_two_pois_and_empty():
    X = _csr([[0], [], [1]], 2)
    tr = BPRTrainer(BPR(3, 2, 4).to(DEV), X)
    for seed in SEEDS:
        want = _bpr_want([[0], [], [1]], [0, 1, 2], 2, seed)
        assert want[2].tolist() == [1, 0]                                  # the other POI
        got = _bpr_direct(X, [0, 1, 2], seed)
        for g, w in zip(list(got[:3]) + _np(tr.batch([0, 1, 2], seed=seed)), want * 2):
            assert np.array_equal(g, w), seed
    assert tr.finish() == 0.0
    # one POI, one user without history: nothing to draw, nothing launched
    tr1 = BPRTrainer(BPR(1, 1, 4).to(DEV), _csr([[]], 1))
    out = tr1.batch([0], seed=3)
    assert all(t.shape == (0,) and t.dtype == torch.int64 for t in out)
    assert tr1.finish() == 0.0


# -------------------------------------------------------------------------------------- GeoIE
# h = 257: nct = 2 column tiles of 256, the second with one live thread; b = 1285 = 80 * 16 + 5,
# a partial last row tile of GT_BR = 16; 1285 candidates, a second sampler pass. h = 256 is the
# exact-tile neighbour (b = 1280 = 80 * 16).
@pytest.mark.parametrize("route", ("dist_mat", "poi_coords"))
@pytest.mark.parametrize("h", (257, 256))
def test_geoie_batch_equals_model(route, h):
    c = shape_case(16, h, 1300)
    ng, P = 4, 1300
    b = h * (1 + ng)
    src = {"dist_mat": c["dm"]} if route == "dist_mat" else {"poi_coords": c["coords"]}
    tr = GeoIETrainer(geoie_model(c["p"], c["a"], c["b"]), c["X"], num_ng=ng, **src)
    row = c["indices"][c["indptr"][1]:c["indptr"][2]]
    cnt = c["data"][c["indptr"][1]:c["indptr"][2]]
    assert len(row) == h
    _poison(*tr.batch(1, seed=1)[1:])                     # the trainer's buffers for this shape
    for seed in SEEDS:
        bufs = tr.batch(1, seed=seed)
        uid, hist, tgt, lab, freq, dist = _np(bufs)
        w_hist, w_tgt, w_lab = sr.nais_batch(row, P, ng, seed)
        assert uid.shape == (b,) and np.all(uid == 1)
        assert np.array_equal(hist, w_hist) and np.array_equal(tgt, w_tgt), seed
        assert lab.dtype == np.float32 and np.array_equal(lab, w_lab)
        # freq by CSR POSITION (batches.py:238-239), whatever POI the shuffle put there
        assert freq.dtype == np.int64 and freq.shape == (b, 1)
        assert np.array_equal(freq.reshape(-1), np.repeat(cnt, 1 + ng))
        assert dist.shape == (b, h)
        if route == "dist_mat":
            want = c["dm"][w_tgt][:, w_hist].astype(np.float32)
            assert np.array_equal(dist.view(np.int32), want.view(np.int32))
        else:
            # every entry written, within one fp32 ulp of the reference's, the clamped ones equal
            want = go.distance_rows(c["coords"], w_tgt, w_hist)
            assert not np.isnan(dist).any() and go.ulp_distance(dist, want).max() <= 1
            cl = (want == np.float32(0.01)) | (want == np.float32(100.0))
            assert np.array_equal(dist[cl], want[cl])
        _poison(*bufs[1:])
    assert tr.finish() == 0.0


@pytest.mark.parametrize("h", (257, 256))
def test_geoie_coordinate_distances_within_one_ulp(h):
    """The coordinate route's whole [b, h] matrix within 1 fp32 ulp of go.distance_rows.

    This catalog has some 60 pairs of POIs closer than 0.3 km, where d = R acos(c) turns a
    relative 2^-53 of c into 2^-53 / angle^2 of d (about 120 fp32 ulps at 25 m). With the device
    libm's sin / cos / acos, which differ from the host's in the last bit, 7 of the 330,245 pairs
    at h = 257 were off by 2 to 97 ulps and 11 of 327,680 at h = 256 by up to 7; the builder now
    rounds the three functions from a double-double evaluation (csrc/nais_geo_cr.h) and every
    pair is within the bound. The figures are printed before the assertion."""
    c = shape_case(16, h, 1300)
    tr = GeoIETrainer(geoie_model(c["p"], c["a"], c["b"]), c["X"], num_ng=4, poi_coords=c["coords"])
    uid, hist, tgt, lab, freq, dist = _np(tr.batch(1, seed=SEEDS[0]))
    want = go.distance_rows(c["coords"], tgt, hist)
    ulp = go.ulp_distance(dist, want)
    print(f"h={h}: {ulp.size} pairs, {(ulp > 1).sum()} off by more than 1 ulp, the worst {ulp.max()} ulps "
          f"at {float(want.reshape(-1)[ulp.argmax()]):.4g} km")
    assert tr.finish() == 0.0
    assert ulp.max() <= 1
