"""GPU: the bounded gather's score intervals against exact scores, at kernel level.

The bounded route returns the exact top-k only if, for every candidate, the interval
that pair_bound_topk_kernel derives from the truncated hi words (make_bounds / upper_score /
lower_score, nais_pairs.hip) contains the fp32 score the refine and nais_pair_gather_topk rank on,
and if the cheap prune (may_reach / lthr_of), the running list of lower keys and the survivor list
never lose a candidate that can still reach the top k. These tests call the C-ABI on hand-built
tables (tests/_pair_bounds.py; no model) and check exactly that:

  exact   nais_pair_gather on the float tables against float64 sigmoid(N / S^beta) of the
          sequential fp32 sums: the exact score every other test here measures against.
  A       one stripe, never-full lists: every candidate's lower key <= exact key <= upper key,
          over input families that stress each margin, the three low-bit patterns of the
          truncation and the widening at both of its ends; and the intervals are not vacuous.
  B       eight stripes: the lower keys and the survivors stay a superset of the exact top-k under
          pruning, compaction, overflow and a job split into ragged column blocks.
  C       the refine returns nais_pair_gather_topk's keys bit for bit; two column shards refined
          under a shared tau merge to the same list.
  D       entry_rows, spans and work change nothing.

Beyond the six input families of the first design, tests/_pair_bounds.py adds two that a shortened
margin needed before any test noticed it (tiny_s: subnormal e with logits of order 1; edge: powers
of two, the truncation margin used up) and the "signed" low-bit patterns and widening modes, which
put N and S at opposite ends of their intervals. The measured figures (pytest -s prints them) are
in the docstrings of test_exact_gather_matches_float64 and test_a_intervals_contain_exact_scores."""
import functools

import numpy as np
import pytest
import torch

import _pair_bounds as pb

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

TIE_ULPS = 4          # the project's figure for fp32 scores of one arithmetic (tests/_helpers.py)
POW_ULPS = 8          # beta != 0.5: twice the measured maximum, rounded up to a power of two (below)
NOKEY = np.uint32(0xFFFFFFFF)   # the score half of a survivor without a finite interval
WIDENS = {"null": None, "zero": (0.0, 0.0), "x3": (4.2e-4, 1e-5), "x1": (5.65e-3, 1e-3), "limit": (2.0 ** -7, 1e-3)}
B_LENGTHS = (0, 1, 2, 3, 4, 5, 7, 16, 17, 31, 33, 63, 64, 65, 66, 90, 100, 127, 128, 129, 130, 150, 160, 170,
             180, 190, 191, 192, 193, 198, 199, 200)
B_P, B_J = 4096, 256


def _lib():
    from poi_recommendation_models_amd import _capi
    return _capi, _capi.load()


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to(DEV)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


class DevJob:
    """A job's CSR on the device, and its column blocks' tables as they are asked for."""

    def __init__(self, job):
        self.job = job
        self.U = len(job["rows"])
        self.rowmap, self.indptr, self.indices = _dev(job["rowmap"]), _dev(job["indptr"]), _dev(job["indices"])
        self.users = _dev(np.arange(self.U, dtype=np.int32))
        self.erows = _dev(job["rowmap"][job["indices"]].astype(np.int32))
        ip = job["indptr"]
        self.spans = _dev(np.stack([ip[:-1], np.diff(ip)], 1).astype(np.int64))
        self._blocks = {}

    def block(self, col0, cols, ld):
        key = (col0, cols, ld)
        if key not in self._blocks:
            self._blocks[key] = tuple(_dev(t) for t in pb.block_tables(self.job, col0, cols, ld))
        return self._blocks[key]   # e, es, ex, hi

    def csr(self):
        return self.rowmap.data_ptr(), self.indptr.data_ptr(), self.indices.data_ptr(), self.users.data_ptr()


def gather_scores(dj, beta):
    """nais_pair_gather over all columns -> (scores float32 [U, P], nan_count)."""
    capi, lib = _lib()
    P = dj.job["P"]
    e, es, _, _ = dj.block(0, P, P)
    out = torch.full((dj.U, P), 7.0, dtype=torch.float32, device=DEV)
    nan = torch.zeros(1, dtype=torch.int32, device=DEV)
    capi.check(lib.nais_pair_gather(e.data_ptr(), es.data_ptr(), P, *dj.csr(), dj.U, 0, P, float(beta),
                                    out.data_ptr(), P, 0, nan.data_ptr(), capi.stream_handle(DEV)), "gather")
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(nan.item())


class Lists:
    def __init__(self, U, k, cap):
        self.k, self.cap = k, cap
        self.lo_keys = torch.zeros(U, k, dtype=torch.int64, device=DEV)
        self.lo_count = torch.zeros(U, dtype=torch.int32, device=DEV)
        self.surv = torch.zeros(U, cap, dtype=torch.int64, device=DEV)
        self.surv_count = torch.zeros(U, dtype=torch.int32, device=DEV)

    def host(self):
        torch.cuda.synchronize()
        return (_u64(self.lo_keys), self.lo_count.cpu().numpy(), _u64(self.surv), self.surv_count.cpu().numpy())


def bound(dj, lists, beta, blocks=None, widen=None, erows=False, spans=False, work=False, plain=False):
    """nais_pair_bound_topk_widened over the column blocks [(col0, cols, ld), ...] (default: all
    columns in one call, ld = P) into `lists`."""
    capi, lib = _lib()
    P = dj.job["P"]
    wd = None if widen is None else _dev(np.asarray(widen, np.float32))
    wk = torch.zeros(1, dtype=torch.int32, device=DEV) if work else None
    for col0, cols, ld in blocks or [(0, P, P)]:
        hi = dj.block(col0, cols, ld)[3]
        head = (hi.data_ptr(), ld, *dj.csr(), dj.U, col0, cols, float(beta), lists.k, lists.lo_keys.data_ptr(),
                lists.lo_count.data_ptr(), lists.surv.data_ptr(), lists.surv_count.data_ptr(), lists.cap,
                dj.erows.data_ptr() if erows else None, dj.spans.data_ptr() if spans else None)
        if plain:
            assert wd is None
            capi.check(lib.nais_pair_bound_topk(*head, capi.ptr(wk), capi.stream_handle(DEV)), "bound")
        else:
            capi.check(lib.nais_pair_bound_topk_widened(*head, capi.ptr(wd), capi.ptr(wk),
                                                        capi.stream_handle(DEV)), "bound_widened")
    return lists.host()


def refine(dj, lists, beta, col0, cols, tau=None, erows=False):
    """nais_pair_refine_topk on the ex table of [col0, col0 + cols) -> (keys, kcount, nan, stats)."""
    capi, lib = _lib()
    ex = dj.block(col0, cols, cols)[2]
    U, k = dj.U, lists.k
    keys = torch.zeros(U, k, dtype=torch.int64, device=DEV)
    kcount = torch.zeros(U, dtype=torch.int32, device=DEV)
    nan = torch.zeros(1, dtype=torch.int32, device=DEV)
    stats = torch.zeros(2, dtype=torch.int32, device=DEV)
    tau_d = None if tau is None else _dev(np.asarray(tau, np.uint64))
    capi.check(lib.nais_pair_refine_topk(
        ex.data_ptr(), dj.job["J"] * 2 * cols, cols, cols, *dj.csr(), U, col0, cols, float(beta), k,
        lists.lo_keys.data_ptr(), lists.lo_count.data_ptr(), lists.surv.data_ptr(), lists.surv_count.data_ptr(),
        lists.cap, capi.ptr(tau_d), keys.data_ptr(), kcount.data_ptr(), nan.data_ptr(), stats.data_ptr(),
        dj.erows.data_ptr() if erows else None, capi.stream_handle(DEV)), "refine")
    torch.cuda.synchronize()
    return _u64(keys), kcount.cpu().numpy(), int(nan.item()), stats.cpu().numpy()


def gather_topk(dj, beta, k):
    capi, lib = _lib()
    P = dj.job["P"]
    e, es, _, _ = dj.block(0, P, P)
    keys = torch.zeros(dj.U, k, dtype=torch.int64, device=DEV)
    kcount = torch.zeros(dj.U, dtype=torch.int32, device=DEV)
    nan = torch.zeros(1, dtype=torch.int32, device=DEV)
    capi.check(lib.nais_pair_gather_topk(e.data_ptr(), es.data_ptr(), P, *dj.csr(), dj.U, 0, P, float(beta), k,
                                         keys.data_ptr(), kcount.data_ptr(), nan.data_ptr(), None,
                                         capi.stream_handle(DEV)), "gather_topk")
    torch.cuda.synchronize()
    return keys, kcount, int(nan.item())


def finish(keys_t, kcount_t, k):
    capi, lib = _lib()
    U = kcount_t.shape[0]
    ids = torch.zeros(U, k, dtype=torch.int32, device=DEV)
    sc = torch.zeros(U, k, dtype=torch.float32, device=DEV)
    short = torch.zeros(1, dtype=torch.int32, device=DEV)
    capi.check(lib.nais_topk_keys_finish(keys_t.data_ptr(), kcount_t.data_ptr(), U, k, ids.data_ptr(),
                                         sc.data_ptr(), short.data_ptr(), capi.stream_handle(DEV)), "finish")
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy().view(np.uint32), int(short.item())


def exact_keys_of(scores):
    """exact key per (user, column) from nais_pair_gather's rows; 0 where the column is no candidate."""
    U, P = scores.shape
    keys = pb.ord_key(scores.ravel(), np.tile(np.arange(P), U)).reshape(U, P)
    return np.where(scores == -1.0, np.uint64(0), keys)


# =================================================================================================
# The exact score
# =================================================================================================
@functools.lru_cache(maxsize=None)
def _a_job(family, pattern, wname, mode, beta):
    return pb.build_job(family, 256, 256, pb.A_LENGTHS, pattern, widen=WIDENS[wname], mode=mode, beta=beta)


@pytest.mark.parametrize("beta", [0.5, 0.7])
@pytest.mark.parametrize("family", pb.FAMILIES + ("clustered", "rising"))
def test_exact_gather_matches_float64(family, beta):
    """nais_pair_gather on the float tables against ref_score(seq_sums(...)) in float64: within
    TIE_ULPS = 4 fp32 ulps at beta = 0.5 and POW_ULPS at beta != 0.5 (powf), NaN exactly where the
    reference is NaN, -1 on the history columns, nan_count the reference's count.

    Measured on an MI355X over all families and patterns: at most 2.269 ulps at beta = 0.5 (edge)
    and 3.092 ulps at beta = 0.7 (edge; 2.214 cancelling, under 2 elsewhere), hence POW_ULPS = 8.
    The families keep their logits within a few units: an fp32 logit is known to 2^-24 |l| at best,
    which exp turns into about |l| half-ulps of a score below 1/2, so no fp32 gather can stay
    within 4 ulps of float64 at l = -10 (a cancelling family with logits down to -10 measured 4.04)."""
    worst = 0.0
    for pattern in pb.PATTERNS:
        job = _a_job(family, pattern, "null", "random", beta)
        ref, cand = pb.exact_reference(job, beta)
        got, nan = gather_scores(DevJob(job), beta)
        assert np.all(got[~cand] == -1.0), "history columns"
        assert np.array_equal(np.isnan(got[cand]), np.isnan(ref[cand])), "NaN where the reference is NaN"
        assert nan == int(np.isnan(ref[cand]).sum())
        d = pb.ulps32(got[cand], ref[cand])
        worst = max(worst, float(d.max()))
        print(f"exact gather {family} {pattern} beta {beta}: max {d.max():.3f} ulps, NaN {nan}")
        assert d.max() <= (TIE_ULPS if beta == 0.5 else POW_ULPS), (family, pattern, float(d.max()))
    print(f"exact gather {family} beta {beta}: worst {worst:.3f} ulps")


# =================================================================================================
# A. Every interval contains the exact score
# =================================================================================================
A_SHARE = {"benign": 1.0, "cancelling": 1.0, "around17": 1.0, "tiny": 0.70, "tiny_s": 0.90, "edge": 1.0,
           "huge": 0.30, "zero": 0.0}
TIGHT = ("benign", "cancelling", "around17")


def _check_intervals(job, beta, res, exact, stat):
    """Per candidate lower key <= exact key <= upper key; returns (finite intervals and candidates of
    the users with a history, lower scores)."""
    lo_keys, lo_count, surv, surv_count = res
    eta, ds = job["widen"] or (0.0, 0.0)
    ek = exact_keys_of(exact)
    fin = tot = 0
    lows = []
    for u, rows in enumerate(job["rows"]):
        cand = np.flatnonzero(ek[u] != 0)
        assert surv_count[u] == cand.size, "a never-full list keeps every candidate as a survivor"
        up = surv[u, :surv_count[u]]
        up_sc, up_id = pb.split_key(up)
        assert np.array_equal(np.sort(up_id), cand), "survivor ids"
        upper = np.zeros(job["P"], np.uint64)
        upper[up_id] = up
        lo = lo_keys[u, :lo_count[u]]
        lo_sc, lo_id = pb.split_key(lo)
        assert len(set(lo_id.tolist())) == lo_id.size
        finite = cand[(upper[cand] >> np.uint64(32)).astype(np.uint32) != NOKEY]
        # no finite interval: absent from lo_keys, present in surv; a finite one: in both
        assert np.array_equal(np.sort(lo_id), finite), "lower keys <-> finite upper keys"
        lower = np.zeros(job["P"], np.uint64)
        lower[lo_id] = lo
        bad_up = cand[upper[cand] < ek[u, cand]]
        bad_lo = finite[lower[finite] > ek[u, finite]]
        for name, bad in (("upper", bad_up), ("lower", bad_lo)):
            if bad.size:
                c = int(bad[0])
                raise AssertionError(
                    f"{job['family']} beta {beta} widen {job['widen']} user {u} (h = {len(rows)}): {bad.size} "
                    f"{name} bounds miss the exact score; column {c}: lower {pb.split_key(lower[c])[0][0]!r} "
                    f"exact {exact[u, c]!r} upper {pb.split_key(upper[c])[0][0]!r}")
        if len(rows) == 0:
            assert np.all(pb.split_key(upper[cand])[0] == 0.5) and np.all(pb.split_key(lower[cand])[0] == 0.5)
            assert np.all(exact[u, cand] == 0.5)
        if len(rows):   # the shares are those of the users with a history
            fin += finite.size
            tot += cand.size
        lows.append(pb.split_key(lower[finite])[0])
        if job["family"] in TIGHT and finite.size:
            ilo, ihi = pb.ideal_interval(job["hi"][rows], beta, eta, ds)
            w = (pb.split_key(upper[finite])[0].astype(np.float64) - pb.split_key(lower[finite])[0])
            iw = (ihi - ilo)[finite]
            assert np.all(np.isfinite(iw))
            assert np.all(w <= 1.10 * iw + 2.0 ** -14), (job["family"], u, float((w - 1.10 * iw).max()))
            big = iw > 1e-3
            if big.any():
                stat["ratio"] = max(stat["ratio"], float((w[big] / iw[big]).max()))
            if (~big).any():
                stat["excess"] = max(stat["excess"], float((w[~big] - iw[~big]).max()))
    return fin, tot, np.concatenate(lows) if lows else np.zeros(0, np.float32)


def _same_lists(a, b):
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[3], b[3])
    for u in range(a[1].size):
        np.testing.assert_array_equal(a[0][u, :a[1][u]], b[0][u, :b[1][u]])
        if a[3][u] >= 0:
            np.testing.assert_array_equal(np.sort(a[2][u, :a[3][u]]), np.sort(b[2][u, :b[3][u]]))


@pytest.mark.parametrize("wname", list(WIDENS))
@pytest.mark.parametrize("beta", [0.5, 0.7])
@pytest.mark.parametrize("family", pb.FAMILIES)
def test_a_intervals_contain_exact_scores(family, beta, wname):
    """One stripe (P = cols = 256, k = 256, surv_cap = 512), histories of 1 .. 200 entries around
    the unroll tail and the 64-entry chunks, and an empty one: no list fills, so lo_keys holds every
    candidate's lower key and surv every candidate's upper key. Per candidate
    lower key <= exact key <= upper key, the exact key being nais_pair_gather's score bits.

    Widths against ideal_interval (benign, cancelling, around 17), asserted <= 1.10 x + 2^-14;
    measured on an MI355X: at most 1.0162 x where the ideal width exceeds 1e-3, at most 1.61e-5
    of absolute excess elsewhere.

    Which input notices which margin (scratch builds of the library with one margin shortened):
    2^-7 -> 2^-8: benign, cancelling, edge, huge, tiny_s ("ones", "signed_*" patterns), and B;
    the l >= 17 shortcut at 16: around 17 (A, B and the refine of C); no ds term: benign,
    cancelling, huge under widening; eta halved: cancelling, edge, tiny_s in the "signed_*" modes
    (not in up / down / random: e and e s move together, so N and S never sit at opposite ends);
    no h 2^-126 term: tiny_s alone. Dropping 3g / 4g, the 2^-19 logit or the 2^-20 score widening
    one at a time is not noticed by any family: the 2^-7 A^ term is never used up (the low half of
    es~ holds e's top bits, at least 1.4 % of it here), and what is left of it covers them."""
    widen = WIDENS[wname]
    stat = {"ratio": 0.0, "excess": 0.0}
    modes = pb.MODES if widen is not None and widen != (0.0, 0.0) else ("random",)
    for pattern in pb.PATTERNS:
        for mode in modes:
            job = _a_job(family, pattern, wname, mode, beta)
            dj = DevJob(job)
            exact, _ = gather_scores(dj, beta)
            res = bound(dj, Lists(dj.U, 256, 512), beta, widen=widen)
            fin, tot, lows = _check_intervals(job, beta, res, exact, stat)
            share = fin / tot
            print(f"A {family} beta {beta} widen {wname} {pattern} {mode}: finite {share:.3f}")
            if family == "zero":
                assert fin == 0
                if pattern == "zeros":
                    hist = np.array([len(r) > 0 for r in job["rows"]])
                    assert np.isnan(exact[hist][exact[hist] != -1.0]).all(), "S = 0: the exact score is NaN"
            else:
                assert share >= A_SHARE[family], (family, pattern, mode, share)
            if family == "around17":
                assert (lows == 1.0).any() and (lows != 1.0).any(), "lower bounds on both sides of the 1.0f shortcut"
            if wname == "zero":   # widen = [0, 0]: the bounds of the unwidened route, bit for bit
                _same_lists(res, bound(dj, Lists(dj.U, 256, 512), beta, widen=None))
            if wname == "null" and pattern == "random":   # the unwidened entry point is the same call
                _same_lists(res, bound(dj, Lists(dj.U, 256, 512), beta, plain=True))
    if family in TIGHT:
        print(f"A {family} beta {beta} widen {wname}: width / ideal <= {stat['ratio']:.4f}, "
              f"absolute excess <= {stat['excess']:.3g}")


# =================================================================================================
# B. Pruning, running lists and survivors across stripes
# =================================================================================================
@functools.lru_cache(maxsize=None)
def _b_job(family, beta, spread=8e-5):
    lengths = tuple(12 + (i % 9) for i in range(8)) if family == "rising" else B_LENGTHS
    # rising: the tables' own low bits (forcing them moves a score by more than a column's step)
    job = pb.build_job(family, B_P, B_J, lengths, "keep" if family == "rising" else "random", seed=1, item_stride=16, item_first=5,
                       shuffle=True, spread=spread, beta=beta)
    dj = DevJob(job)
    exact, _ = gather_scores(dj, beta)
    exact.setflags(write=False)
    return job, dj, exact


def _check_superset(job, k, res, exact, overflow_ok=False):
    """The assertions of B on one job's lists; returns the users whose survivor list overflowed."""
    lo_keys, lo_count, surv, surv_count = res
    ek = exact_keys_of(exact)
    over = []
    for u in range(len(job["rows"])):
        cand = np.flatnonzero(ek[u] != 0)
        top = np.sort(ek[u, cand])[::-1][:k]
        assert lo_count[u] == min(k, cand.size), (u, lo_count[u], cand.size)
        lo = lo_keys[u, :lo_count[u]]
        _, lo_id = pb.split_key(lo)
        assert len(set(lo_id.tolist())) == lo_id.size, "an id twice in lo_keys"
        assert np.all(ek[u, lo_id] != 0), "a history column in lo_keys"
        assert np.all(lo <= ek[u, lo_id]), (u, "a lower key above its exact key")
        assert np.all(lo[1:] < lo[:-1]), "lo_keys descending"
        if lo_count[u] == k:
            assert lo[k - 1] <= top[k - 1], (u, "the k-th lower key above the k-th exact key")
        if surv_count[u] == -1:
            assert overflow_ok, (u, "survivor list overflowed")
            over.append(u)
            continue
        sv = surv[u, :surv_count[u]]
        _, sv_id = pb.split_key(sv)
        assert len(set(sv_id.tolist())) == sv_id.size, "an id twice in surv"
        assert np.all(ek[u, sv_id] != 0), "a history column in surv"
        assert np.all(sv >= ek[u, sv_id]), (u, "an upper key below its exact key")
        _, top_id = pb.split_key(top)
        missing = np.setdiff1d(top_id, sv_id)
        assert missing.size == 0, (u, "exact top-k members dropped", missing[:8].tolist())
    return over


B_FAMILIES = ("benign", "cancelling", "around17", "clustered")


@pytest.mark.parametrize("k", [1, 8, 50, 256])
@pytest.mark.parametrize("beta", [0.5, 0.7])
@pytest.mark.parametrize("family", B_FAMILIES)
def test_b_lists_keep_the_exact_topk(family, beta, k):
    """P = 4096 in one call (8 stripes in stream order), 32 users, h <= 200, surv_cap = 1024."""
    job, dj, exact = _b_job(family, beta)
    if family == "clustered":
        c = exact[exact != -1.0]
        assert np.all(np.abs(c - 0.5) <= 1e-4)
    res = bound(dj, Lists(dj.U, k, 1024), beta)
    _check_superset(job, k, res, exact)
    print(f"B {family} beta {beta} k {k}: survivors per user mean {res[3].mean():.1f} max {res[3].max()}")


@pytest.mark.parametrize("beta", [0.5, 0.7])
def test_b_compaction_without_overflow(beta):
    """Exact scores rise with the column id, k = 16, surv_cap = 64: every stripe's best candidates
    beat all before them, so a list that was never compacted would pass the cap."""
    k, cap = 16, 64
    job, dj, exact = _b_job("rising", beta)
    ek = exact_keys_of(exact)
    for u in range(dj.U):
        c = exact[u][exact[u] != -1.0]
        assert np.all(np.diff(c.astype(np.float64)) > 0), "scores rise with the column"
        n = 0   # per stripe: the candidates that reach the k-th exact key of the columns so far
        for s0 in range(0, B_P, 512):
            sofar = ek[u, :s0 + 512]
            kth = np.sort(sofar[sofar != 0])[::-1][k - 1]
            n += int((ek[u, s0:s0 + 512] >= kth).sum())
        assert n > cap, (u, n)
    res = bound(dj, Lists(dj.U, k, cap), beta)
    _check_superset(job, k, res, exact)
    assert np.all((res[3] >= k) & (res[3] <= cap)), res[3]
    print(f"B rising beta {beta}: survivor counts {res[3].tolist()}")


def test_b_overflow_keeps_the_lower_keys_sound():
    k, cap = 60, 64
    job, dj, exact = _b_job("clustered", 0.5, 2e-6)
    assert np.all(np.abs(exact[exact != -1.0] - 0.5) <= 1e-4)
    res = bound(dj, Lists(dj.U, k, cap), 0.5)
    over = _check_superset(job, k, res, exact, overflow_ok=True)
    assert over, "no user overflowed"
    print(f"B overflow: {len(over)} of {dj.U} users overflowed")


SPLIT = [(0, 1500), (1500, 1), (1501, B_P - 1501)]


@pytest.mark.parametrize("k", [8, 256])
@pytest.mark.parametrize("beta", [0.5, 0.7])
@pytest.mark.parametrize("family", B_FAMILIES)
def test_b_ragged_column_blocks(family, beta, k):
    """The same job as three calls, col0 no multiple of 512 and ld > cols."""
    job, dj, exact = _b_job(family, beta)
    blocks = [(c0, w, (w + 4) // 4 * 4) for c0, w in SPLIT]
    res = bound(dj, Lists(dj.U, k, 1024), beta, blocks=blocks)
    _check_superset(job, k, res, exact)


# =================================================================================================
# C. Refine, and tau in one process
# =================================================================================================
@pytest.mark.parametrize("beta", [0.5, 0.7])
@pytest.mark.parametrize("family", B_FAMILIES + ("rising",))
def test_c_refine_equals_exact_gather_topk(family, beta):
    job, dj, exact = _b_job(family, beta)
    ncand = (exact != -1.0).sum(1)
    for k in (8, 256):
        lists = Lists(dj.U, k, 1024)
        bound(dj, lists, beta)
        keys, kcount, nan, stats = refine(dj, lists, beta, 0, B_P)
        xk, xc, xnan = gather_topk(dj, beta, k)
        want, wc = _u64(xk), xc.cpu().numpy()
        np.testing.assert_array_equal(kcount, wc)
        np.testing.assert_array_equal(kcount, np.minimum(k, ncand))
        for u in range(dj.U):
            np.testing.assert_array_equal(keys[u, :kcount[u]], want[u, :wc[u]])
            ek = exact_keys_of(exact[u:u + 1])[0]
            np.testing.assert_array_equal(want[u, :wc[u]], np.sort(ek[ek != 0])[::-1][:k])
        a = finish(_dev(keys), _dev(kcount), k)
        b = finish(xk, xc, k)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
        assert stats[0] >= int(np.minimum(k, ncand).sum()) and stats[1] == 0
        assert nan == 0 and xnan == 0
        print(f"C {family} beta {beta} k {k}: refined {stats[0] / dj.U:.1f} per user")


@pytest.mark.parametrize("beta", [0.5, 0.7])
@pytest.mark.parametrize("family", ["benign", "clustered", "rising"])
def test_c_two_shards_share_tau(family, beta):
    """Two column shards with their own lists; tau[u] = the k-th largest lower key of both. Each
    shard refined under tau returns only ids whose upper key reaches it, and the two lists merge to
    the single-shard exact list. In the rising job the second shard holds every winner."""
    k, half = 50, B_P // 2
    job, dj, exact = _b_job(family, beta)
    shards = []
    for c0 in (0, half):
        lists = Lists(dj.U, k, 1024)
        shards.append((c0, lists, bound(dj, lists, beta, blocks=[(c0, half, half)])))
    tau = np.zeros(dj.U, np.uint64)
    for u in range(dj.U):
        both = np.concatenate([r[0][u, :r[1][u]] for _, _, r in shards])
        if both.size >= k:
            tau[u] = np.sort(both)[::-1][k - 1]
    want, wc, _ = gather_topk(dj, beta, k)
    want, wc = _u64(want), wc.cpu().numpy()
    got, short = [], 0
    for c0, lists, res in shards:
        keys, kcount, _, _ = refine(dj, lists, beta, c0, half, tau=tau)
        assert np.all(res[3] >= 0)
        for u in range(dj.U):
            sv = res[2][u, :res[3][u]]
            upper = dict(zip(pb.split_key(sv)[1].tolist(), sv.tolist()))
            ids = pb.split_key(keys[u, :kcount[u]])[1]
            assert np.all((ids >= c0) & (ids < c0 + half))
            assert all(upper[int(i)] >= int(tau[u]) for i in ids), (u, "an id whose upper key is below tau")
        short += int((kcount < k).sum())
        got.append((keys, kcount))
    for u in range(dj.U):
        merged = np.sort(np.concatenate([ks[u, :kc[u]] for ks, kc in got]))[::-1][:k]
        np.testing.assert_array_equal(merged, want[u, :wc[u]])
    assert short > 0, "no shard returned a short list"
    if family == "rising":
        assert np.all(got[0][1] == 0), "the first shard holds no winner"
    print(f"C shards {family} beta {beta}: {short} short lists of {2 * dj.U}")


# =================================================================================================
# D. Same results with and without the optional inputs
# =================================================================================================
@pytest.mark.parametrize("k", [8, 256])
@pytest.mark.parametrize("family", ["benign", "clustered"])
def test_d_optional_inputs_change_nothing(family, k):
    job, dj, exact = _b_job(family, 0.5)
    base = bound(dj, Lists(dj.U, k, 1024), 0.5)
    _check_superset(job, k, base, exact)
    for opt in (dict(erows=True, spans=True), dict(erows=True), dict(spans=True), dict(work=True),
                dict(erows=True, spans=True, work=True)):
        _same_lists(base, bound(dj, Lists(dj.U, k, 1024), 0.5, **opt))
