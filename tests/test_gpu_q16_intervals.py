"""GPU: the bounded gather from q16 blocks (nais_pair_bound_topk_q16, ABI 20) against exact scores.

The A / B / C / D plan of tests/test_gpu_bound_intervals.py (whose helpers, jobs' families and
checks this file reuses), on the same hand-built float tables, quantised to q16 blocks by the
reference quantiser of tests/_q16_format.py (the tabled pair (et, est) is quantised; the exact
tables (e, es) are what the exact gather and the refine sum):

  A   one stripe, never-full lists: lower key <= exact key <= upper key for every candidate, over
      every input family, low-bit pattern and widening mode, with the widening at zero, at the
      one-product values and at its limit; the finite intervals equal the numpy port's
      (tests/_q16_format.interval_q16) to 2^-18 of score.
  B   P = 4096, J = 256: lists and survivors stay a superset of the exact top-k under pruning,
      compaction (surv_cap = 64) and overflow, in one block of ld = 4096 (8 stripes, the stripe
      offset inside a block) and cut into column blocks of 512, 1, 15, 16, 17, 511, 512, ... columns.
  C   nais_pair_refine_topk's keys after a q16 gather equal nais_pair_gather_topk's bit for bit.
  D   entry_rows, spans and work change nothing.

History lengths 0, 1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129 and 200 occur in every job: the q16 row
loop steps by 8 rows, inside chunks of 64 entries. Padding columns of every block hold 0xFF bytes
(NaN scales): a gather that summed one would lose its candidates' finite intervals, and the
survivor ids are checked to be candidates.

The tiny, tiny_s, edge and zero families get no finite interval from q16 blocks (scales stop at
2^-100: include/nais.h); their candidates must all survive, which A asserts."""
import functools

import numpy as np
import pytest
import torch

import _pair_bounds as pb
import _q16_format as qf
import test_gpu_bound_intervals as bi

pytestmark = pytest.mark.gpu
DEV = bi.DEV
LENGTHS = (1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 200, 0)
WIDENS = {"zero": (0.0, 0.0), "x1": (5.65e-3, 1e-3), "limit": (2.0 ** -7, 1e-3)}
# finite intervals among the candidates of users with a history, at least. A candidate has none when
# every m_e of its history is 0 (e below 1 / 255 of its group's largest): never around 17 (e within
# 5 % of 1), and for a ~ N(., 1) that takes a value 5.5 below the group's largest, less than 1e-4 of
# the entries. Nothing is promised where the sums leave fp32's range or e lies below the scales' floor.
A_SHARE = {"benign": 0.99, "cancelling": 0.99, "around17": 1.0, "tiny": 0.0, "tiny_s": 0.0, "edge": 0.0,
           "huge": 0.0, "zero": 0.0}


class QJob(bi.DevJob):
    def q16(self, col0, cols, ld):
        key = ("q16", col0, cols, ld)
        if key not in self._blocks:
            sl = slice(col0, col0 + cols)
            self._blocks[key] = torch.from_numpy(qf.quantise(self.job["et"][:, sl], self.job["est"][:, sl], ld)).to(DEV)
        return self._blocks[key]


def bound_q16(dj, lists, beta, blocks=None, widen=(0.0, 0.0), erows=False, spans=False, work=False):
    capi, lib = bi._lib()
    P = dj.job["P"]
    wd = None if widen is None else bi._dev(np.asarray(widen, np.float32))
    wk = torch.zeros(1, dtype=torch.int32, device=DEV) if work else None
    for col0, cols, ld in blocks or [(0, P, P)]:
        blk = dj.q16(col0, cols, ld)
        capi.check(lib.nais_pair_bound_topk_q16(
            blk.data_ptr(), ld, qf.pitch(ld), *dj.csr(), dj.U, col0, cols, float(beta), lists.k,
            lists.lo_keys.data_ptr(), lists.lo_count.data_ptr(), lists.surv.data_ptr(),
            lists.surv_count.data_ptr(), lists.cap, dj.erows.data_ptr() if erows else None,
            dj.spans.data_ptr() if spans else None, capi.ptr(wd), capi.ptr(wk), capi.stream_handle(DEV)),
            "bound_q16")
    return lists.host()


# =================================================================================================
# A
# =================================================================================================
@functools.lru_cache(maxsize=None)
def _a_job(family, pattern, wname, mode, beta):
    job = pb.build_job(family, 256, 256, LENGTHS, pattern, widen=WIDENS[wname], mode=mode, beta=beta)
    dj = QJob(job)
    exact, _ = bi.gather_scores(dj, beta)
    exact.setflags(write=False)
    return job, dj, exact


def _check_a(job, beta, res, exact, port):
    """lower <= exact <= upper per candidate; returns (finite, candidates) over users with a history."""
    lo_keys, lo_count, surv, surv_count = res
    ek = bi.exact_keys_of(exact)
    eta, ds = job["widen"]
    fin = tot = 0
    for u, rows in enumerate(job["rows"]):
        cand = np.flatnonzero(ek[u] != 0)
        assert surv_count[u] == cand.size, "a never-full list keeps every candidate as a survivor"
        up = surv[u, :surv_count[u]]
        up_id = pb.split_key(up)[1]
        assert np.array_equal(np.sort(up_id), cand), "survivor ids are the candidates"
        upper = np.zeros(job["P"], np.uint64)
        upper[up_id] = up
        lo = lo_keys[u, :lo_count[u]]
        lo_id = pb.split_key(lo)[1]
        finite = cand[(upper[cand] >> np.uint64(32)).astype(np.uint32) != bi.NOKEY]
        assert np.array_equal(np.sort(lo_id), finite), "lower keys <-> finite upper keys"
        lower = np.zeros(job["P"], np.uint64)
        lower[lo_id] = lo
        for name, bad in (("upper", cand[upper[cand] < ek[u, cand]]), ("lower", finite[lower[finite] > ek[u, finite]])):
            if bad.size:
                c = int(bad[0])
                raise AssertionError(
                    f"{job['family']} beta {beta} widen {job['widen']} user {u} (h = {len(rows)}): {bad.size} "
                    f"{name} bounds miss the exact score; column {c}: lower {pb.split_key(lower[c])[0][0]!r} "
                    f"exact {exact[u, c]!r} upper {pb.split_key(upper[c])[0][0]!r}")
        if len(rows) == 0:
            assert np.all(pb.split_key(upper[cand])[0] == 0.5) and np.all(pb.split_key(lower[cand])[0] == 0.5)
            continue
        fin += finite.size
        tot += cand.size
        if port and finite.size:   # the kernel's interval is the documented one
            me, ms, qe, qs = port
            S, N, Qe, Qs = qf.seq_sums_q16(me[rows], ms[rows], qe[rows], qs[rows])
            plo, pup, ok = qf.interval_q16(S, N, Qe, Qs, len(rows), beta, eta, ds)
            assert np.array_equal(np.flatnonzero(ok & (ek[u] != 0)), finite), "finite where the port is"
            d = max(np.abs(pb.split_key(lower[finite])[0].astype(np.float64) - plo[finite]).max(),
                    np.abs(pb.split_key(upper[finite])[0].astype(np.float64) - pup[finite]).max())
            assert d <= 2.0 ** -18, (u, d)
    return fin, tot


@pytest.mark.parametrize("wname", list(WIDENS))
@pytest.mark.parametrize("beta", [0.5, 0.7])
@pytest.mark.parametrize("family", pb.FAMILIES)
def test_a_q16_intervals_contain_exact_scores(family, beta, wname):
    """P = cols = ld = 256, k = 256, surv_cap = 512: no list fills. Measured finite shares on an
    MI355X are printed (pytest -s)."""
    widen = WIDENS[wname]
    modes = pb.MODES if widen != (0.0, 0.0) else ("random",)
    for pattern in pb.PATTERNS:
        for mode in modes:
            job, dj, exact = _a_job(family, pattern, wname, mode, beta)
            res = bound_q16(dj, bi.Lists(dj.U, 256, 512), beta, widen=widen)
            port = None
            if family == "benign" and mode == "random":
                port = qf.dequantise(dj.q16(0, 256, 256).cpu().numpy(), 256, 256)
            fin, tot = _check_a(job, beta, res, exact, port)
            print(f"A q16 {family} beta {beta} widen {wname} {pattern} {mode}: finite {fin / tot:.3f}")
            assert fin / tot >= A_SHARE[family], (family, pattern, mode, fin / tot)
            if family == "zero":
                assert fin == 0


@pytest.mark.parametrize("beta", [0.5, 0.7])
def test_a_q16_ragged_blocks_keep_finite_intervals(beta):
    """The A job cut into blocks of 17 (ld 20), 1 (ld 4) and 238 columns: the last 16-byte load of
    a row is only partly inside the block, and its valid columns must still be read (a range check
    that zeroed the whole load would leave S^ = 0 there: no finite interval, everything refined,
    and no superset test would notice). Around 17 every e is within 5 % of 1, so every candidate's
    interval is finite whatever the cut."""
    job, dj, exact = _a_job("around17", "random", "x1", "random", beta)
    res = bound_q16(dj, bi.Lists(dj.U, 256, 512), beta, blocks=[(0, 17, 20), (17, 1, 4), (18, 238, 238)],
                    widen=WIDENS["x1"])
    fin, tot = _check_a(job, beta, res, exact, None)
    assert fin == tot, (fin, tot)


# =================================================================================================
# B, C, D
# =================================================================================================
B_P, B_J = bi.B_P, bi.B_J
B_LENGTHS = LENGTHS + (3, 4, 5, 16, 17, 31, 33, 66, 90, 100, 130, 150, 160, 190, 191, 192, 193, 198, 199)
CUTS = (512, 1, 15, 16, 17, 511, 512)


def _blocks():
    out, c0 = [], 0
    for w in CUTS + (512,) * 8:
        w = min(w, B_P - c0)
        if w <= 0:
            break
        out.append((c0, w, w))
        c0 += w
    assert c0 == B_P
    return out


@functools.lru_cache(maxsize=None)
def _b_job(family, beta, spread=8e-5):
    lengths = tuple(12 + (i % 9) for i in range(8)) if family == "rising" else B_LENGTHS
    job = pb.build_job(family, B_P, B_J, lengths, "keep" if family == "rising" else "random", seed=1,
                       item_stride=16, item_first=5, shuffle=True, spread=spread, beta=beta)
    dj = QJob(job)
    exact, _ = bi.gather_scores(dj, beta)
    exact.setflags(write=False)
    return job, dj, exact


@pytest.mark.parametrize("k", [1, 50, 256])
@pytest.mark.parametrize("beta", [0.5, 0.7])
@pytest.mark.parametrize("family", bi.B_FAMILIES)
def test_b_q16_lists_keep_the_exact_topk(family, beta, k):
    job, dj, exact = _b_job(family, beta)
    one = bound_q16(dj, bi.Lists(dj.U, k, 1024), beta)
    bi._check_superset(job, k, one, exact)
    cut = bound_q16(dj, bi.Lists(dj.U, k, 1024), beta, blocks=_blocks())
    bi._check_superset(job, k, cut, exact)
    print(f"B q16 {family} beta {beta} k {k}: survivors per user mean {one[3].mean():.1f} max {one[3].max()}; "
          f"cut into {len(_blocks())} blocks mean {cut[3].mean():.1f}")


@pytest.mark.parametrize("beta", [0.5, 0.7])
def test_b_q16_compaction_without_overflow(beta):
    k, cap = 16, 64
    job, dj, exact = _b_job("rising", beta)
    res = bound_q16(dj, bi.Lists(dj.U, k, cap), beta, blocks=_blocks())
    over = bi._check_superset(job, k, res, exact, overflow_ok=True)
    print(f"B q16 rising beta {beta}: survivor counts {res[3].tolist()}")
    # every stripe's best beat all before them (bi.test_b_compaction_without_overflow shows more than
    # cap candidates pass uncompacted), so a list within the cap was compacted
    assert np.any((res[3] >= k) & (res[3] <= cap)), res[3]


def test_b_q16_overflow_keeps_the_lower_keys_sound():
    k, cap = 60, 64
    job, dj, exact = _b_job("clustered", 0.5, 2e-6)
    res = bound_q16(dj, bi.Lists(dj.U, k, cap), 0.5)
    over = bi._check_superset(job, k, res, exact, overflow_ok=True)
    assert over, "no user overflowed"


@pytest.mark.parametrize("beta", [0.5, 0.7])
@pytest.mark.parametrize("family", bi.B_FAMILIES + ("rising",))
def test_c_q16_refine_equals_exact_gather_topk(family, beta):
    job, dj, exact = _b_job(family, beta)
    ncand = (exact != -1.0).sum(1)
    for k, blocks in ((8, None), (256, _blocks())):
        lists = bi.Lists(dj.U, k, 1024)
        bound_q16(dj, lists, beta, blocks=blocks)
        keys, kcount, nan, stats = bi.refine(dj, lists, beta, 0, B_P)
        xk, xc, xnan = bi.gather_topk(dj, beta, k)
        want, wc = bi._u64(xk), xc.cpu().numpy()
        np.testing.assert_array_equal(kcount, wc)
        np.testing.assert_array_equal(kcount, np.minimum(k, ncand))
        for u in range(dj.U):
            np.testing.assert_array_equal(keys[u, :kcount[u]], want[u, :wc[u]])
        assert nan == 0 and xnan == 0
        print(f"C q16 {family} beta {beta} k {k}: refined {stats[0] / dj.U:.1f} per user, overflowed {stats[1]}")


@pytest.mark.parametrize("k", [8, 256])
@pytest.mark.parametrize("family", ["benign", "clustered"])
def test_d_q16_optional_inputs_change_nothing(family, k):
    job, dj, exact = _b_job(family, 0.5)
    base = bound_q16(dj, bi.Lists(dj.U, k, 1024), 0.5)
    for opt in (dict(erows=True, spans=True), dict(erows=True), dict(spans=True), dict(work=True),
                dict(erows=True, spans=True, work=True), dict(widen=None)):
        bi._same_lists(base, bound_q16(dj, bi.Lists(dj.U, k, 1024), 0.5, **opt))
