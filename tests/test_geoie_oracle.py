"""The numpy GeoIE oracle (tests/_geoie_oracle.py) against the reference fixture
(tests/golden/geoie.npz, captured by tests/golden/make_golden_geoie.py), and the fixture's own
conditions: the measured tie window and no tie run straddling a cut-off under it. The oracle
alone passes every assertion the GPU tests make (tests/test_gpu_geoie.py)."""
import numpy as np
import pytest

import _geoie_oracle as go
from _helpers import SCORE_ATOL, assert_metrics_exact, assert_topk_equivalent, straddles

ORACLE_ATOL = 1e-6   # the project's oracle bar
TAGS = ("init", "spread")

# (tag, user, k) whose reference top-k has a tie run straddling k under go.TIE_ULPS
STRADDLING = set()


@pytest.fixture(scope="module")
def fx():
    return go.fixture()


def test_fixture_hits_both_clamps_and_history_lengths(fx):
    dm = fx["dist_mat"]
    assert dm[0, 1] == 0.01 and dm[2, 3] == 0.01 and dm.min() == 0.01      # co-located, < 10 m
    assert np.all(np.delete(dm[4], 4) == 100.0) and dm.max() == 100.0      # the far POI
    assert 0.01 < np.median(dm) < 100.0
    D = fx["D"]
    lens = np.diff(fx["indptr"]).tolist()
    assert {1, 2, D} <= set(lens)
    assert any(h % D and D % h for h in lens if h > D) and any(D % h for h in lens if 2 < h < D)
    hist_all = set(fx["indices"].tolist())
    assert {0, 1, 2, 3, 4} <= hist_all


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("n", (1, 7, 33))
def test_forward_batches(fx, tag, n):
    z, t = fx["z"], fx["tags"][tag]
    pre = f"{tag}/fwd{n}/"
    hist = z[pre + "history"]
    assert np.all(hist == hist[0])
    # the recorded float32 distances are dist_mat[target, history] rebuilt from the coordinates
    dist = fx["dist_mat"][z[pre + "target"]][:, hist[0]].astype(np.float32)
    np.testing.assert_array_equal(dist, z[pre + "distances"])
    got = go.forward(t["p"], t["a"], t["b"], z[pre + "user"], z[pre + "target"], hist[0], dist)
    assert got.shape == (n,) and z[pre + "prediction"].shape == (n, 1)
    assert np.max(np.abs(got - z[pre + "prediction"][:, 0])) <= ORACLE_ATOL
    w = go.wuj(z[pre + "freq"])
    assert w.shape == (n, 1) and w.dtype == np.float32
    np.testing.assert_array_equal(w.view(np.int32), z[pre + "wuj"].view(np.int32))


def test_measured_ulp_distance_and_tie_window(fx):
    """M: the largest fp32-ulp distance between the reference's and the oracle's catalog scores."""
    worst = 0
    for tag in TAGS:
        ref, ours = fx["z"][f"{tag}/rows"], fx["tags"][tag]["rows"]
        assert np.array_equal(ref < 0, ours < 0)
        cand = ref >= 0
        assert np.max(np.abs(ref[cand] - ours[cand])) <= ORACLE_ATOL
        m = int(go.ulp_distance(ref[cand], ours[cand]).max())
        print(f"{tag}: max ulp distance {m}, max abs {np.max(np.abs(ref[cand] - ours[cand])):.3g}")
        worst = max(worst, m)
    assert worst == go.M_ULPS
    assert go.TIE_ULPS == max(4, 2 * go.M_ULPS)


@pytest.mark.parametrize("tag", TAGS)
def test_no_tie_run_straddles_a_cutoff(fx, tag):
    z = fx["z"]
    found = {(tag, u, k) for u in range(fx["U"]) for k in fx["k_list"]
             if straddles(z[f"{tag}/topk_scores"][u], k, go.TIE_ULPS)}
    assert found == {s for s in STRADDLING if s[0] == tag}


@pytest.mark.parametrize("tag", TAGS)
def test_topk_lists_and_metrics(fx, tag):
    from oracle import metrics_oracle
    z, rows = fx["z"], fx["tags"][tag]["rows"]
    ref_ids, ref_sc = z[f"{tag}/topk_ids"], z[f"{tag}/topk_scores"]
    ours = []
    for u in range(fx["U"]):
        cand = np.flatnonzero(rows[u] >= 0)
        ids, sc = go.topk(cand, rows[u, cand], 50)
        lut = {int(c): float(z[f"{tag}/rows"][u, c]) for c in ids}
        assert_topk_equivalent(ref_ids[u], ref_sc[u], ids, sc, score_atol=SCORE_ATOL, lookup=lut,
                               tie_ulps=go.TIE_ULPS)
        ours.append(ids.tolist())
    got = []
    for pos in (fx["val"], fx["test"]):
        got.extend(metrics_oracle.evaluate(pos, ours, fx["k_list"]))
    excused = assert_metrics_exact(got, ref_ids, ref_sc, ours, fx["val"], fx["test"], fx["k_list"],
                                   tie_ulps=go.TIE_ULPS)
    assert {(tag, u, k) for u, k in excused} == {s for s in STRADDLING if s[0] == tag}
    np.testing.assert_array_equal(np.array(got), z[f"{tag}/metrics"])


@pytest.mark.parametrize("tag", TAGS)
def test_training_batch_prediction_and_loss(fx, tag):
    z, t = fx["z"], fx["tags"][tag]
    pre = f"{tag}/train/"
    hist = z[pre + "history"]
    assert np.all(hist == hist[0]) and len(z[pre + "target"]) == 5 * hist.shape[1]
    pred = go.forward(t["p"], t["a"], t["b"], z[pre + "user"], z[pre + "target"], hist[0],
                      z[pre + "distances"])
    assert np.max(np.abs(pred - z[pre + "prediction"][:, 0])) <= ORACLE_ATOL
    w = go.wuj(z[pre + "freq"])
    np.testing.assert_array_equal(w.view(np.int32), z[pre + "wuj"].view(np.int32))
    loss = go.loss_function(pred[:, None], z[pre + "label"][:, None], w)
    assert abs(float(loss) - float(z[pre + "loss"])) <= 1e-6 * abs(float(z[pre + "loss"]))


def test_empty_history_and_short_catalog_raise(fx):
    t = fx["tags"]["init"]
    with pytest.raises(ValueError):
        go.forward(t["p"], t["a"], t["b"], [0], [5], [], np.zeros((1, 0), np.float32))
    cand = np.arange(10)
    with pytest.raises(RuntimeError):
        go.topk(cand, np.zeros(10, np.float32), 11)
