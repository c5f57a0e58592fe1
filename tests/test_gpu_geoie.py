"""GeoIE on the device (model.GeoIE, validation.GeoIE_validation, geoie.score_topk) against the
reference fixture tests/golden/geoie.npz and, for shapes the fixture does not hold, against the
numpy oracle tests/_geoie_oracle.py (itself pinned to the fixture by tests/test_geoie_oracle.py)."""
import numpy as np
import pytest
import scipy.sparse as sp

import _geoie_oracle as go
from _helpers import GRAD_RTOL, SCORE_ATOL, assert_metrics_exact, assert_topk_equivalent

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from poi_recommendation_models_amd import geoie  # noqa: E402
from poi_recommendation_models_amd.model import GeoIE  # noqa: E402
from poi_recommendation_models_amd.validation import GeoIE_validation  # noqa: E402

DEV = "cuda:0"
TAGS = ("init", "spread")
W = go.TIE_ULPS


class Args:
    topk = 50


def make_model(p, a, b):
    U, D = p["UserPreference.weight"].shape
    P = p["PoiPreference.weight"].shape[0]
    m = GeoIE(U, P, D, 4, a, b)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in p.items()})
    return m.to(DEV)


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).to(DEV)


@pytest.fixture(scope="module")
def fx():
    return go.fixture()


# ------------------------------------------------------------------------------- golden
@pytest.mark.parametrize("tag", TAGS)
def test_golden_forward(fx, tag):
    z, t = fx["z"], fx["tags"][tag]
    m = make_model(t["p"], t["a"], t["b"]).eval()
    for n in (1, 7, 33):
        pre = f"{tag}/fwd{n}/"
        with torch.no_grad():
            pred, w = m(dev(z[pre + "user"]), dev(z[pre + "target"]), dev(z[pre + "history"]),
                        dev(z[pre + "freq"]), dev(z[pre + "distances"]))
        assert tuple(pred.shape) == (n, 1) and tuple(w.shape) == (n, 1) and w.dtype == torch.float32
        d = np.max(np.abs(pred.cpu().numpy() - z[pre + "prediction"]))
        print(f"{tag} n={n}: max |dpred| {d:.3g}")
        assert d <= SCORE_ATOL
        # two fp32 logs (the device's and the host's, each within an ulp or so) and the add's rounding
        assert go.ulp_distance(w.cpu().numpy(), z[pre + "wuj"]).max() <= 4


@pytest.mark.parametrize("route", ("dist_mat", "poi_coords"))
@pytest.mark.parametrize("tag", TAGS)
def test_golden_validation(fx, tag, route):
    z, t = fx["z"], fx["tags"][tag]
    m = make_model(t["p"], t["a"], t["b"])
    X = go.train_matrix(fx)
    kw = dict(dist_mat=fx["dist_mat"]) if route == "dist_mat" else dict(coords=fx["coords"])
    ids, sc, rows = geoie.score_topk(m, X, range(fx["U"]), 50, return_rows=True, **kw)
    ids, sc, rows = ids.cpu().numpy(), sc.cpu().numpy(), rows.cpu().numpy()
    ref_rows = z[f"{tag}/rows"]
    assert np.array_equal(rows < 0, ref_rows < 0) and np.all(rows[ref_rows < 0] == -1.0)
    d = np.max(np.abs(rows - ref_rows))
    print(f"{tag} {route}: max |dscore| {d:.3g}, max ulps "
          f"{go.ulp_distance(rows[ref_rows >= 0], ref_rows[ref_rows >= 0]).max()}")
    assert d <= SCORE_ATOL
    ref_ids, ref_sc = z[f"{tag}/topk_ids"], z[f"{tag}/topk_scores"]
    for u in range(fx["U"]):
        lut = {int(c): float(ref_rows[u, c]) for c in ids[u]}
        assert_topk_equivalent(ref_ids[u], ref_sc[u], ids[u], sc[u], lookup=lut, tie_ulps=W)
    if route == "dist_mat":
        got = GeoIE_validation(m, Args(), fx["U"], fx["test"], fx["val"], X, fx["k_list"], fx["dist_mat"])
    else:
        got = GeoIE_validation(m, Args(), fx["U"], fx["test"], fx["val"], X, fx["k_list"], None,
                               poi_coords=fx["coords"])
    assert len(got) == 6
    excused = assert_metrics_exact(got, ref_ids, ref_sc, ids, fx["val"], fx["test"], fx["k_list"],
                                   tie_ulps=W)
    assert excused == []
    np.testing.assert_array_equal(np.array(got), z[f"{tag}/metrics"])


# ------------------------------------------------------------------- shapes vs the oracle
def _numpy_dist_mat(coords):
    """A clamped great-circle matrix (vectorised; any positive matrix is a valid dist_mat input:
    the device and the oracle both read THIS one), [candidate, history]."""
    phi = np.radians(90.0 - coords[:, 0])
    th = np.radians(coords[:, 1])
    cosv = np.sin(phi)[:, None] * np.sin(phi)[None] * np.cos(th[:, None] - th[None]) + \
        np.cos(phi)[:, None] * np.cos(phi)[None]
    d = np.arccos(np.clip(cosv, -1.0, 1.0)) * 6371.0
    return np.minimum(np.maximum(0.01, d), 100.0)


_cases = {}


def shape_case(D, P):
    """Seeded model + histories for one (D, P): users with h in {1, 2, 31, 32, 33, 65, 300, D} and
    one user with exactly 50 candidates; the oracle's rows computed once and shared."""
    if (D, P) in _cases:
        return _cases[(D, P)]
    rng = np.random.default_rng(1000 * D + P)
    lens = [1, 2, 31, 32, 33, 65, 300] + ([D] if D not in (1, 2, 31, 32, 33, 65, 300) else []) + [P - 50]
    U = len(lens)
    coords = np.stack([35.5 + 0.3 * rng.random(P), 139.4 + 0.4 * rng.random(P)], 1)
    coords[1] = coords[0]
    indptr, indices = [0], []
    for h in lens:
        indices.extend(np.sort(rng.choice(P, h, replace=False)).tolist())
        indptr.append(len(indices))
    indptr, indices = np.array(indptr, np.int64), np.array(indices, np.int64)
    p = {n: (0.3 * rng.standard_normal((U if n.startswith("User") else P, D))).astype(np.float32)
         for n in go.PARAM_NAMES}
    a, b = 0.8, -0.9
    dm = _numpy_dist_mat(coords)
    rows = np.full((U, P), -1.0, dtype=np.float32)
    for u in range(U):
        cand, sc = go.catalog_scores(p, a, b, u, indices[indptr[u]:indptr[u + 1]], P, dist_mat=dm)
        rows[u, cand] = sc
    rows.setflags(write=False)
    X = sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(U, P))
    c = dict(D=D, P=P, U=U, lens=np.array(lens), coords=coords, indptr=indptr, indices=indices, p=p,
             a=a, b=b, dm=dm, rows=rows, X=X)
    _cases[(D, P)] = c
    return c


def _check_lists(c, users, ids, sc, k):
    for i, u in enumerate(users):
        cand = np.flatnonzero(c["rows"][u] >= 0)
        rid, rsc = go.topk(cand, c["rows"][u, cand], k)
        lut = {int(x): float(c["rows"][u, x]) for x in ids[i]}
        assert_topk_equivalent(rid, rsc, ids[i], sc[i], lookup=lut, tie_ulps=W)


# every D in {1, 8, 20, 64, 100, 128} with every h in {1, 2, 31, 32, 33, 65, 300} and h == D
# (h < D, h > D coprime to D among them); P = 301 in one block, P = 1,002 in two 501-column blocks.
# D = 256 (the widest the entry points take) is the one shape at which the scorer runs two waves
# per workgroup instead of four, so it is here too, at the small catalog.
@pytest.mark.parametrize("D,P,block", [(1, 301, None), (8, 1002, 501), (20, 301, None),
                                       (64, 1002, 501), (100, 301, 77), (128, 1002, 501),
                                       (256, 301, 77)])
def test_shapes_catalog_and_forward(D, P, block):
    c = shape_case(D, P)
    m = make_model(c["p"], c["a"], c["b"]).eval()
    U, lens = c["U"], c["lens"]
    everyone = np.arange(U)
    # k = 1 for every user (the h = 300 user of P = 301 has one candidate)
    ids1, sc1, rows = geoie.score_topk(m, c["X"], everyone, 1, dist_mat=c["dm"], block_cols=block,
                                       return_rows=True)
    rows = rows.cpu().numpy()
    assert np.array_equal(rows < 0, c["rows"] < 0) and np.all(rows[c["rows"] < 0] == -1.0)
    d = np.max(np.abs(rows - c["rows"]))
    print(f"D={D} P={P}: max |dscore| vs oracle {d:.3g}")
    assert d <= SCORE_ATOL
    _check_lists(c, everyone, ids1.cpu().numpy(), sc1.cpu().numpy(), 1)
    # the coordinates route forms its own float64 distances: same rows within the score tolerance
    rows_c = geoie.score_topk(m, c["X"], everyone, 1, coords=c["coords"], block_cols=block,
                              return_rows=True)[2].cpu().numpy()
    assert np.max(np.abs(rows_c - c["rows"])) <= SCORE_ATOL
    # k = 50: every user with at least 50 candidates, the one with exactly 50 among them
    u50 = everyone[P - lens >= 50]
    assert (P - lens == 50).any()
    ids50, sc50 = geoie.score_topk(m, c["X"], u50, 50, dist_mat=c["dm"], block_cols=block)
    ids50, sc50 = ids50.cpu().numpy(), sc50.cpu().numpy()
    _check_lists(c, u50, ids50, sc50, 50)
    exact = int(np.flatnonzero(P - lens[u50] == 50)[0])
    assert sorted(ids50[exact].tolist()) == np.flatnonzero(c["rows"][u50[exact]] >= 0).tolist()
    # k = 256, the users in groups of 3 (each group lists its own history POIs and table rows)
    u256 = everyone[P - lens >= 256]
    if len(u256):
        ids256, sc256 = geoie.score_topk(m, c["X"], u256, 256, dist_mat=c["dm"], block_cols=block,
                                         group_users=3)
        _check_lists(c, u256, ids256.cpu().numpy(), sc256.cpu().numpy(), 256)
    # k greater than a user's candidate count raises, as torch.topk does
    with pytest.raises(RuntimeError):
        geoie.score_topk(m, c["X"], everyone, 51, dist_mat=c["dm"], block_cols=block)
    # catalog winners re-scored by the forward kernel (the tensors the reference's forward receives)
    worst = 0
    for i, u in enumerate(u50):
        hist = c["indices"][c["indptr"][u]:c["indptr"][u + 1]]
        tg = ids50[i]
        dist = c["dm"][tg][:, hist].astype(np.float32)
        with torch.no_grad():
            pred, _ = m(dev(np.full(len(tg), u, np.int64)), dev(tg), dev(np.tile(hist, (len(tg), 1))),
                        dev(np.ones((len(tg), 1), np.int64)), dev(dist))
        pred = pred.cpu().numpy()[:, 0]
        assert np.max(np.abs(pred - c["rows"][u, tg])) <= SCORE_ATOL
        worst = max(worst, int(go.ulp_distance(pred, sc50[i]).max()))
    print(f"D={D} P={P}: forward vs catalog winners, max ulps {worst}")
    assert worst <= 2


def test_empty_history_raises():
    c = shape_case(8, 1002)
    m = make_model(c["p"], c["a"], c["b"]).eval()
    indptr = np.concatenate([c["indptr"][:3], [c["indptr"][2]], c["indptr"][3:]])   # user 2: empty
    X = sp.csr_matrix((np.ones(len(c["indices"])), c["indices"], indptr), shape=(c["U"] + 1, c["P"]))
    p = dict(c["p"])
    p["UserPreference.weight"] = np.concatenate([p["UserPreference.weight"]] * 2)[:c["U"] + 1]
    m2 = make_model(p, c["a"], c["b"]).eval()
    with pytest.raises(ValueError, match="user 2"):
        geoie.score_topk(m2, X, range(c["U"] + 1), 1, dist_mat=c["dm"])
    with pytest.raises(ValueError, match="user"):
        GeoIE_validation(m2, Args(), c["U"] + 1, [[]] * (c["U"] + 1), [[]] * (c["U"] + 1), X, [5],
                         c["dm"])
    with torch.no_grad(), pytest.raises(ValueError, match="user 3"):
        m(dev(np.array([3], np.int64)), dev(np.array([5], np.int64)),
          torch.zeros(1, 0, dtype=torch.int64, device=DEV), dev(np.ones((1, 1), np.int64)),
          torch.zeros(1, 0, dtype=torch.float32, device=DEV))


def test_off_device_raises(fx):
    t = fx["tags"]["init"]
    U, D = t["p"]["UserPreference.weight"].shape
    m = GeoIE(U, fx["P"], D, 4, t["a"], t["b"])
    assert m.scaling == 10 and m.negnum == 4 and m.POI_count == fx["P"]
    assert set(m.state_dict()) == set(go.PARAM_NAMES)
    i = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="ROCm"):
        m(i, i, torch.zeros(1, 1, dtype=torch.int64), torch.ones(1, 1, dtype=torch.int64), torch.ones(1, 1))


# ------------------------------------------------------------------------------- clamps
@pytest.mark.parametrize("tag", TAGS)
def test_clamped_table_entries(fx, tag):
    t = fx["tags"][tag]
    m = make_model(t["p"], t["a"], t["b"])
    P, items = fx["P"], [0, 1, 2, 3, 4]            # co-located pair, < 10 m pair, the far POI
    dm = fx["dist_mat"]
    assert dm[1, 0] == 0.01 and dm[3, 2] == 0.01 and dm[7, 4] == 100.0
    d32 = dev(dm[:, items].T, torch.float32)                       # [item, candidate] = dm[c, item]
    want = float(t["a"]) * (d32 ** float(t["b"]))                  # torch on the device
    F = geoie.pair_table(m, items, 0, P, dist_mat=dm)
    assert torch.equal(F.view(torch.int32), want.view(torch.int32))
    # an odd block of columns that starts off a multiple of 4
    F2 = geoie.pair_table(m, items, 3, 201, dist_mat=dm)
    assert torch.equal(F2, F[:, 3:204])
    # coordinates: the device distance is within one fp32 ulp of the reference's (DESIGN (c)), so
    # f moves by at most |b| ulps, plus the rounding of powf and of the multiply on either side
    Fc = geoie.pair_table(m, items, 0, P, coords=fx["coords"]).cpu().numpy().astype(np.float64)
    wn = want.cpu().numpy().astype(np.float64)
    rel = np.max(np.abs(Fc - wn) / wn)
    print(f"{tag}: coords table max rel {rel:.3g}")
    assert rel <= (abs(t["b"]) + 2) * 2.0 ** -23
    clamped = (dm[:, items].T == 0.01) | (dm[:, items].T == 100.0)
    assert clamped.sum() > P and np.array_equal(Fc[clamped], wn[clamped])


# ---------------------------------------------------------------------------------- NaN
def test_nan_row_in_geosusceptibility(fx):
    t = fx["tags"]["spread"]
    X = go.train_matrix(fx)
    m = make_model(t["p"], t["a"], t["b"])
    base = geoie.score_topk(m, X, range(fx["U"]), 1, dist_mat=fx["dist_mat"], return_rows=True)[2].cpu().numpy()
    cstar = 150
    p = {k: v.copy() for k, v in t["p"].items()}
    p["GeoSusceptibility.weight"][cstar] = np.nan
    m2 = make_model(p, t["a"], t["b"])
    ids, sc, rows = geoie.score_topk(m2, X, range(fx["U"]), 1, dist_mat=fx["dist_mat"], block_cols=77,
                                     return_rows=True)
    rows = rows.cpu().numpy()
    cand = base[:, cstar] >= 0
    assert cand.sum() >= fx["U"] - 1
    assert np.all(np.isnan(rows[cand, cstar])) and np.all(rows[~cand, cstar] == -1.0)
    others = np.delete(np.arange(fx["P"]), cstar)
    assert np.array_equal(rows[:, others].view(np.int32), base[:, others].view(np.int32))
    assert np.all(ids.cpu().numpy()[cand, 0] == cstar) and np.all(np.isnan(sc.cpu().numpy()[cand, 0]))
    assert int(m2._last_nan.item()) == int(cand.sum())


# ------------------------------------------------------------------------- training path
@pytest.mark.parametrize("tag", TAGS)
def test_training_path(fx, tag):
    z, t = fx["z"], fx["tags"][tag]
    pre = f"{tag}/train/"
    m = make_model(t["p"], t["a"], t["b"]).train()
    args = [dev(z[pre + k]) for k in ("user", "target", "history", "freq", "distances")]
    pred, w = m(*args)
    assert pred.requires_grad and tuple(pred.shape) == (len(z[pre + "target"]), 1)
    loss = m.loss_function(pred, dev(z[pre + "label"]).unsqueeze(1), w)
    loss.backward()
    assert np.max(np.abs(pred.detach().cpu().numpy() - z[pre + "prediction"])) <= SCORE_ATOL
    ref_loss = float(z[pre + "loss"])
    assert abs(loss.item() - ref_loss) <= 1e-5 * abs(ref_loss)
    for n, prm in m.named_parameters():
        g, r = prm.grad.cpu().numpy(), z[pre + "grad/" + n]
        assert np.max(np.abs(g - r)) <= GRAD_RTOL * np.max(np.abs(r)), n
    with torch.no_grad():
        hip, w2 = m(*args)
    assert not hip.requires_grad and torch.equal(w2, w)
    assert np.max(np.abs(hip.cpu().numpy() - pred.detach().cpu().numpy())) <= 1e-6


# -------------------------------------------------------------------------- memory shape
def test_large_catalog_allocates_nothing_p_by_p():
    P, U, D = 20000, 8, 16
    rng = np.random.default_rng(3)
    coords = np.stack([35.5 + 0.3 * rng.random(P), 139.4 + 0.4 * rng.random(P)], 1)
    indptr, indices = [0], []
    for u in range(U):
        indices.extend(np.sort(rng.choice(P, 10 + 7 * u, replace=False)).tolist())
        indptr.append(len(indices))
    X = sp.csr_matrix((np.ones(len(indices)), np.array(indices), np.array(indptr)), shape=(U, P))
    p = {n: (0.3 * rng.standard_normal((U if n.startswith("User") else P, D))).astype(np.float32)
         for n in go.PARAM_NAMES}
    m = make_model(p, 0.8, -0.9)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ids, sc = geoie.score_topk(m, X, range(U), 50, coords=coords)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"peak allocated {peak / 1e6:.1f} MB")
    assert peak < 1e9                       # a P x P float64 matrix alone would be 3.2 GB
    ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
    assert np.all(np.diff(sc, axis=1) <= 0) and np.all((sc >= 0) & (sc <= 1))
    for u in range(U):
        assert len(set(ids[u])) == 50 and not set(ids[u]) & set(indices[indptr[u]:indptr[u + 1]])
    # one user's winners against the oracle
    cand, ref = go.catalog_scores(p, 0.8, -0.9, 0, indices[:indptr[1]], P, coords=coords)
    lut = dict(zip(cand.tolist(), ref.tolist()))
    assert np.max(np.abs(np.array([lut[int(c)] for c in ids[0]]) - sc[0])) <= SCORE_ATOL
