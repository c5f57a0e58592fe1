"""CPU: the numpy helpers of tests/_pair_bounds.py that tests/test_gpu_bound_intervals.py leans on.

Keys order and round-trip as include/nais.h states; pack_hi holds the identities that
test_gpu_bounded.py::test_split_tables_hold_the_float_bits asserts of the split16 kernels;
seq_sums is a plain loop; and every input family yields the share of finite intervals the GPU test
relies on. That share comes from an fp32 numpy restatement of make_bounds (nais_pairs.hip) that
lives here only: the GPU tests never use it as a reference."""
import numpy as np
import pytest

import _pair_bounds as pb

F32 = np.float32


def test_keys_order_and_round_trip():
    nan = F32(np.nan)
    vals = np.array([-np.inf, -1.0, -0.0, 0.0, 1e-45, 0.5, np.nextafter(F32(1), F32(0)), 1.0, np.inf, nan], F32)
    keys = pb.ord_key(vals, np.full(vals.size, 7))
    assert np.all(keys[1:] > keys[:-1]), "ascending scores (-0.0 < +0.0, NaN above +inf) -> ascending keys"
    sc, poi = pb.split_key(keys)
    np.testing.assert_array_equal(sc.view(np.uint32)[:-1], vals.view(np.uint32)[:-1])   # -0.0 keeps its sign
    assert np.isnan(sc[-1]) and np.all(poi == 7)
    # every NaN payload and sign is the one key
    odd = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], np.uint32).view(F32)
    assert len(set(pb.ord_key(odd, np.zeros(4)).tolist())) == 1
    # ties: the smaller id ranks higher; the id half never carries into the score half
    for v in (F32(0.5), F32(1.0), F32(-0.0), nan):
        k = pb.ord_key(np.full(3, v, F32), np.array([0, 5, 0xFFFFFFFF]))
        assert k[0] > k[1] > k[2]
        assert len(set((k >> np.uint64(32)).tolist())) == 1
        np.testing.assert_array_equal(pb.split_key(k)[1], [0, 5, 0xFFFFFFFF])
    assert pb.ord_key(F32(0.5), 0xFFFFFFFF)[0] > pb.ord_key(np.nextafter(F32(0.5), F32(0)), 0)[0]
    assert int(pb.ord_key(F32(0.5), 3)[0]) == (0xBF000000 << 32) | (0xFFFFFFFF - 3)
    assert np.all(pb.ord_key(vals, np.arange(vals.size)) > 0), "0 is no valid key"


def test_pack_hi_holds_the_float_bits():
    rng = np.random.default_rng(0)
    e = rng.integers(0, 1 << 32, 4096, dtype=np.uint32).view(F32)
    es = rng.integers(0, 1 << 32, 4096, dtype=np.uint32).view(F32)
    hi = pb.pack_hi(e, es)
    np.testing.assert_array_equal(hi << np.uint32(16), e.view(np.uint32) & np.uint32(0xFFFF0000))
    np.testing.assert_array_equal(hi & np.uint32(0xFFFF0000), es.view(np.uint32) & np.uint32(0xFFFF0000))
    eh, st = pb.hi_values(hi)
    np.testing.assert_array_equal(eh.view(np.uint32), e.view(np.uint32) & np.uint32(0xFFFF0000))
    np.testing.assert_array_equal(st.view(np.uint32), hi)
    # the truncation contract on finite positive e and any finite es
    e = np.exp(rng.uniform(-60, 60, 4096)).astype(F32)   # e, e*s in the normal range
    es = (e * rng.normal(0, 1, 4096)).astype(F32)
    eh, st = pb.hi_values(pb.pack_hi(e, es))
    assert np.all((eh <= e) & (e.astype(np.float64) < eh.astype(np.float64) * (1 + 2.0 ** -7)))
    assert np.all(np.abs(es.astype(np.float64) - st) < 2.0 ** -7 * np.abs(st.astype(np.float64)))
    assert np.all(np.signbit(st) == np.signbit(es))


def test_seq_sums_is_the_plain_loop():
    rng = np.random.default_rng(1)
    e = np.exp(rng.normal(0, 3, (37, 5))).astype(F32)
    es = (e * rng.normal(0, 1, (37, 5))).astype(F32)
    S, N = pb.seq_sums(e, es)
    for c in range(5):
        s = n = F32(0)
        for j in range(37):
            s = F32(s + e[j, c])
            n = F32(n + es[j, c])
        assert s == S[c] and n == N[c]
    assert S.dtype == F32 and N.dtype == F32
    S0, N0 = pb.seq_sums(e[:0], es[:0])
    assert S0.shape == (5,) and not S0.any() and not N0.any()
    # order matters in fp32: the helper must not sort or pair
    big = np.array([[1e8], [1.0], [-1e8]], F32)
    assert pb.seq_sums(big, big)[0][0] == F32(0) and pb.seq_sums(big[[0, 2, 1]], big[[0, 2, 1]])[0][0] == F32(1)


def test_ref_score_cases():
    S = np.array([4.0, 0.0, np.inf, 0.0, 1e-40, 4.0], F32)
    N = np.array([2.0, 0.0, np.inf, 1.0, 1e-40, -np.inf], F32)
    r = pb.ref_score(S, N, 0.5)
    assert abs(r[0] - 1 / (1 + np.exp(-1.0))) < 1e-15
    assert np.isnan(r[1]) and np.isnan(r[2]) and r[3] == 1.0 and abs(r[4] - 0.5) < 1e-15 and r[5] == 0.0
    assert np.all(pb.ref_score(S, N, 0.5, empty=True) == 0.5)
    b32 = float(F32(0.7))   # the kernels take beta as a float32
    assert abs(pb.ref_score(F32(8.0), F32(2.0), 0.7) - 1 / (1 + np.exp(-2.0 / 8.0 ** b32))) < 1e-15


def _make_bounds_f32(S, N, A, hl, beta, eta, ds):
    """make_bounds of nais_pairs.hip, operation by operation in np.float32 -> ok mask."""
    with np.errstate(all="ignore"):
        one = F32(1)
        eta, ds = F32(eta), F32(ds)
        eta2 = F32(eta * F32(1.02) + F32(2.0 ** -21)) if eta > 0 else F32(0)
        g = F32(F32(hl) * F32(2.0 ** -23) + F32(2.0 ** -20))
        tiny = F32(F32(hl) * F32(2.0 ** -126))
        g3, g4, t7 = F32(F32(3) * g), F32(F32(4) * g), F32(2.0 ** -7)
        slo = S * (one - g3) * (one - eta)
        su = S * (one + t7)
        shi = su * (one + g3) * (one + eta) + tiny
        rn = (t7 + g4 + eta2) * A + (tiny + su * (one + eta) * ds)
        nlo, nhi = N - rn, N + rn
        if beta == 0.5:
            dlo, dhi = np.sqrt(slo), np.sqrt(shi)
        else:
            p0, p1 = np.power(slo, F32(beta)), np.power(shi, F32(beta))
            dlo, dhi = np.minimum(p0, p1), np.maximum(p0, p1)
        for x in (slo, shi, rn, nlo, dlo):
            assert x.dtype == F32
        return (slo > 0) & (dlo > 0) & np.isfinite(dhi) & np.isfinite(nlo) & np.isfinite(nhi)


def _finite_share(job, beta):
    eta, ds = job["widen"] or (0.0, 0.0)
    ok = tot = 0
    for rows in job["rows"]:
        if len(rows) == 0:
            continue
        eh, st = pb.hi_values(job["hi"][rows])
        S, N = pb.seq_sums(eh, st)
        A, _ = pb.seq_sums(np.abs(st), st)
        cand = np.ones(job["P"], bool)
        cand[job["items"][rows]] = False
        ok += int(_make_bounds_f32(S, N, A, len(rows), beta, eta, ds)[cand].sum())
        tot += int(cand.sum())
    return ok / tot


SHARE = {"benign": (1.0, 1.0), "cancelling": (1.0, 1.0), "around17": (1.0, 1.0), "tiny": (0.70, 1.0),
         "tiny_s": (0.90, 1.0), "edge": (1.0, 1.0), "huge": (0.30, 1.0), "zero": (0.0, 0.0)}
WIDENS = (None, (4.2e-4, 1e-5), (2.0 ** -7, 1e-3))


@pytest.mark.parametrize("family", pb.FAMILIES)
def test_family_share_of_finite_intervals(family):
    lo, hi = SHARE[family]
    for pattern in pb.PATTERNS:
        for widen in WIDENS:
            for beta in (0.5, 0.7):
                job = pb.build_job(family, 256, 256, pb.A_LENGTHS, pattern, widen=widen, mode="up")
                sh = _finite_share(job, beta)
                print(family, pattern, widen, beta, "finite share %.3f" % sh)
                assert lo <= sh <= hi, (family, pattern, widen, beta, sh)


@pytest.mark.parametrize("family", ("benign", "cancelling", "around17", "clustered", "rising"))
def test_builders_keep_the_contract(family):
    """The exact float64 score of the exact tables lies in ideal_interval of the hi words (up to the
    fp32 rounding of the sums, which the ideal interval leaves out), in every widening mode; the
    widened tables stay within eta of the tabled e."""
    for widen in (None, (0.0, 0.0), (5.65e-3, 1e-3)):
        for mode in pb.MODES:
            job = pb.build_job(family, 256, 256, pb.A_LENGTHS, "random", widen=widen, mode=mode)
            eta, ds = widen or (0.0, 0.0)
            e64, t64 = job["e"].astype(np.float64), job["et"].astype(np.float64)
            assert np.all(np.abs(e64 - t64) <= eta * t64)
            if eta == 0.0:
                assert job["e"] is job["et"] and job["es"] is job["est"]
            else:
                assert (job["e"] != job["et"]).mean() > 0.99
            sc, cand = pb.exact_reference(job, 0.5)
            for u, rows in enumerate(job["rows"]):
                lo, hi = pb.ideal_interval(job["hi"][rows], 0.5, eta, ds)
                c = cand[u]
                assert np.all(np.isfinite(lo[c]) & (lo[c] - 1e-5 <= sc[u][c]) & (sc[u][c] <= hi[c] + 1e-5))
                if len(rows) == 0:
                    assert np.all(lo == 0.5) and np.all(hi == 0.5) and np.all(sc[u] == 0.5)


def test_block_tables_layout():
    job = pb.build_job("benign", 256, 256, (3, 0), "random")
    e, es, ex, hi = pb.block_tables(job, 100, 37, 40)
    assert e.shape == (256, 40) and ex.shape == (256, 80) and hi.dtype == np.uint32
    np.testing.assert_array_equal(e[:, :37], job["e"][:, 100:137])
    np.testing.assert_array_equal(ex[:, 0:74:2], e[:, :37].view(np.uint32))
    np.testing.assert_array_equal(ex[:, 1:74:2], es[:, :37].view(np.uint32))
    np.testing.assert_array_equal(hi[:, :37], pb.pack_hi(e[:, :37], es[:, :37]))
    assert np.isnan(e[:, 37:]).all() and np.isnan(es[:, 37:]).all()
    assert np.array_equal(job["rowmap"][job["items"]], np.arange(256))
    assert job["indptr"].tolist() == [0, 3, 3] and np.all(np.diff(job["indices"]) > 0)
