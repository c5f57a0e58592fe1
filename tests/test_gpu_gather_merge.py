"""GPU: the bounded gather's lists, counts and survivors against a numpy replay, both table formats.

What a visit (one user, one stripe of <= 512 columns) does with its candidates' score intervals is
fixed by include/nais.h: the keys offered are the lower keys above the list's k-th key, the new
list is the k best of list and offered keys in descending order, tau is its k-th key once it is
full, the visit's survivors are the candidates whose upper key is >= tau, in column order, and a
survivor list that would pass surv_cap is first compacted by tau and marked -1 if it still does
not fit. The intervals themselves do not depend on the lists, so a pass with lists that never
fill (k = 256 over at most 256 columns, surv_cap = 512) returns every candidate's upper and lower
key, and `replay` below turns those into the lists any k, cut and cap must give, key for key.

That pins down the two things the merge and the pruning threshold may not change: the sorted list
(merge by rank for a few offered keys, bitonic sort for many) and the survivor set (a threshold
logit set too high would drop a candidate whose upper key reaches tau). The replay also counts
the keys offered per visit; the tests assert that 0, 1, MERGE_INS = 8, 9 and more than 256 (a whole
first block) occur, so both merges and their boundary run.

Threshold jobs: the k-th score at 0.5, at 1.0f, just below 1 and at 1e-30, each approached by
candidates whose upper scores step through it in the smallest steps the table can express. The
tables for that are found with the gather itself, on hi words: the sum N of a candidate is a
coarse term plus three finer ones on further history rows (each an integer below 256 times a step
128 times smaller than the last, so hi words hold them exactly; the last steps N by 1 / 32 of its
fp32 ulp), and a never-full pass per level picks the value just under the k-th key. Measured on an
MI355X the upper scores then lie -2 .. 2 ulps around the k-th score at 0.5, -2 .. 0 at 1.0f and just
below 1, and -339 .. 473 at 1e-30 (where one ulp of N moves the score by 64). The q16 gather
replays the same tables; its intervals are wider, so its candidates sit further below the k-th
score (printed with pytest -s), and the check there is the replay alone."""
import functools

import numpy as np
import pytest
import torch

import _pair_bounds as pb
import _q16_format as qf
import test_gpu_bound_intervals as bi
import test_gpu_q16_intervals as qi

pytestmark = pytest.mark.gpu
MERGE_INS = 8
FORMATS = ("hi", "q16")
KS = (1, 50, 64, 65, 256)


def _run(fmt, dj, lists, beta, blocks):
    if fmt == "q16":
        return qi.bound_q16(dj, lists, beta, blocks=blocks)
    return bi.bound(dj, lists, beta, blocks=blocks)


def _b(c0, w):
    return (c0, w, (w + 3) // 4 * 4)   # the hi table's pitch is a multiple of 4 words


def _sub256(blocks):
    """Every block cut again at multiples of 256 columns from its start (q16 groups of 16 columns
    count from the block's start, so the pieces hold the words of the whole block)."""
    return [(c0, w, [(c0 + o, min(256, w - o)) for o in range(0, w, 256)]) for c0, w, _ in blocks]


def intervals(fmt, dj, beta, blocks):
    """(upper, lower) keys uint64 [U, P] of every candidate of the blocks' columns, 0 where a column
    is no candidate (upper) or has no finite interval (lower), from never-full passes."""
    P, U = dj.job["P"], dj.U
    upper = np.zeros((U, P), np.uint64)
    lower = np.zeros((U, P), np.uint64)
    for c0, w, pieces in _sub256(blocks):
        for p0, pw in pieces:
            lists = bi.Lists(U, 256, 512)
            res = _q16_piece(dj, p0, pw, lists, beta) if fmt == "q16" else bi.bound(dj, lists, beta, blocks=[_b(p0, pw)])
            lo_keys, lo_count, surv, surv_count = res
            for u in range(U):
                s = surv[u, :surv_count[u]]
                upper[u, pb.split_key(s)[1]] = s
                l = lo_keys[u, :lo_count[u]]
                lower[u, pb.split_key(l)[1]] = l
    return upper, lower


def _q16_piece(dj, p0, pw, lists, beta):
    """nais_pair_bound_topk_q16 on columns [p0, p0 + pw) quantised on their own: the quantiser works
    per row and 16-column group, and a piece starts a multiple of 16 columns into its block, so
    these are the words the whole block holds for those columns."""
    capi, lib = bi._lib()
    sl = slice(p0, p0 + pw)
    piece = torch.from_numpy(qf.quantise(dj.job["et"][:, sl], dj.job["est"][:, sl], pw)).to(bi.DEV)
    wd = bi._dev(np.asarray((0.0, 0.0), np.float32))
    capi.check(lib.nais_pair_bound_topk_q16(
        piece.data_ptr(), pw, qf.pitch(pw), *dj.csr(), dj.U, p0, pw, float(beta), lists.k,
        lists.lo_keys.data_ptr(), lists.lo_count.data_ptr(), lists.surv.data_ptr(),
        lists.surv_count.data_ptr(), lists.cap, None, None, capi.ptr(wd), None,
        capi.stream_handle(bi.DEV)), "bound_q16")
    return lists.host()


def replay(upper, lower, blocks, k, cap):
    """The lists of one user after the blocks' visits -> (list, survivors or None when overflowed,
    offered keys per visit)."""
    lst = np.zeros(0, np.uint64)
    surv, over, offered = [], False, []
    for c0, w, _ in blocks:
        for s0 in range(c0, c0 + w, 512):
            cols = np.arange(s0, min(s0 + 512, c0 + w))
            up, lo = upper[cols], lower[cols]
            thr = lst[k - 1] if lst.size == k else np.uint64(0)
            off = lo[(lo != 0) & (lo > thr)]
            offered.append(off.size)
            lst = np.sort(np.concatenate([lst, off]))[::-1][:k]
            tau = lst[k - 1] if lst.size == k else np.uint64(0)
            new = up[(up != 0) & (up >= tau)]
            if new.size and not over:
                if len(surv) + new.size > cap:
                    surv = [v for v in surv if v >= tau]
                    over = len(surv) + new.size > cap
                if not over:
                    surv.extend(new.tolist())
    return lst, (None if over else np.asarray(surv, np.uint64)), offered


def check(fmt, dj, beta, blocks, k, cap, upper, lower):
    """The gather's lists equal the replay's; returns (offered counts, overflowed users)."""
    lo_keys, lo_count, surv, surv_count = _run(fmt, dj, bi.Lists(dj.U, k, cap), beta, blocks)
    offered, nover = [], 0
    for u in range(dj.U):
        lst, sv, off = replay(upper[u], lower[u], blocks, k, cap)
        offered += off
        assert lo_count[u] == lst.size, (fmt, k, u, lo_count[u], lst.size)
        np.testing.assert_array_equal(lo_keys[u, :lst.size], lst, err_msg=f"{fmt} k {k} user {u}: list")
        if sv is None:
            nover += 1
            assert surv_count[u] == -1, (fmt, k, u, surv_count[u])
        else:
            assert surv_count[u] == sv.size, (fmt, k, u, surv_count[u], sv.size)
            np.testing.assert_array_equal(surv[u, :sv.size], sv, err_msg=f"{fmt} k {k} user {u}: survivors")
    return offered, nover


# ---- lists, counts, survivors over families, k, cuts and caps ------------------------------------
P, J = 2048, 256
LENGTHS = (0, 1, 2, 7, 8, 9, 63, 64, 65, 100, 100, 100, 128, 129, 200, 33, 50, 90, 150, 16)
WHOLE = [_b(c0, 512) for c0 in range(0, P, 512)]                  # the first visit offers every column
NARROW = [_b(c0, 128) for c0 in range(0, P, 128)]                 # lists not yet full for k = 256
RAGGED = [_b(0, 37), _b(37, 1), _b(38, 16), _b(54, 511), _b(565, 17), _b(582, 700), _b(1282, P - 1282)]
CUTS = {"whole": WHOLE, "narrow": NARROW, "ragged": RAGGED}


@functools.lru_cache(maxsize=None)
def _job(family, fmt, cut):
    job = pb.build_job(family, P, J, LENGTHS, "keep" if family == "rising" else "random", seed=3,
                       item_stride=8, item_first=3, shuffle=True, spread=2e-6)
    dj = qi.QJob(job)
    upper, lower = intervals(fmt, dj, 0.5, CUTS[cut])
    upper.setflags(write=False)
    lower.setflags(write=False)
    return dj, upper, lower


@pytest.fixture(scope="module", autouse=True)
def _release_device_jobs():
    """The cached jobs hold device tables: dropped with the module, so that tests which measure
    allocated device memory see none of it."""
    yield
    _job.cache_clear()
    _threshold_tables.cache_clear()


@pytest.mark.parametrize("cut", list(CUTS))
@pytest.mark.parametrize("fmt", FORMATS)
def test_lists_and_survivors_equal_the_replay(fmt, cut):
    """benign: distinct scores; k of 1, 50, 64, 65 and 256 (more on the narrow cut); a cap that never binds."""
    dj, upper, lower = _job("benign", fmt, cut)
    seen = set()
    for k in KS + ((8, 16, 24, 32) if cut == "narrow" else ()):
        offered, nover = check(fmt, dj, 0.5, CUTS[cut], k, 4096, upper, lower)
        assert nover == 0
        seen |= set(offered)
        print(f"{fmt} {cut} k {k}: (keys offered, visits): {sorted((o, offered.count(o)) for o in set(offered))[:24]}")
    if cut == "narrow":   # the merge by rank at nothing, one key and its limit; one more: the sort
        assert {0, 1, MERGE_INS, MERGE_INS + 1} <= seen, sorted(seen)[:16]
    if cut == "whole":    # a first block in which every column offers takes both 256-key sorts
        assert max(seen) > 256, max(seen)


@pytest.mark.parametrize("fmt", FORMATS)
def test_equal_scores_differ_by_id(fmt):
    """clustered at 2e-6: scores collide in fp32, so the id halves order the keys."""
    dj, upper, lower = _job("clustered", fmt, "narrow")
    sc = pb.split_key(lower[5][lower[5] != 0])[0]
    assert np.unique(sc).size < sc.size, "no two lower scores equal"
    for k in (50, 256):
        check(fmt, dj, 0.5, NARROW, k, 4096, upper, lower)


@pytest.mark.parametrize("fmt", FORMATS)
def test_compaction_and_overflow(fmt):
    """rising: each stripe's best beat all before them, so survivor lists grow past a small cap and
    are compacted; clustered under a cap of 64 overflows."""
    dj, upper, lower = _job("rising", fmt, "narrow")
    free = _run(fmt, dj, bi.Lists(dj.U, 16, 4096), 0.5, NARROW)[3]
    offered, nover = check(fmt, dj, 0.5, NARROW, 16, 256, upper, lower)
    got = _run(fmt, dj, bi.Lists(dj.U, 16, 256), 0.5, NARROW)[3]
    print(f"{fmt} rising: survivors uncapped {free.tolist()}, under cap 256 {got.tolist()}")
    assert np.any((free > 256) & (got >= 0)), "no list was compacted and kept"
    dj, upper, lower = _job("clustered", fmt, "narrow")
    offered, nover = check(fmt, dj, 0.5, NARROW, 60, 64, upper, lower)
    assert nover > 0, "no user overflowed"


# ---- the pruning threshold -----------------------------------------------------------------------
# One user per target: history rows (A, B, C, D) of its own, e = 1 on all four (S = 4, logit N / 2).
# Columns 0 .. 255: N = n1 on row A alone, so the list fills with one lower score (ids break the
# ties) and tau is its key. Columns 256 .. 511: N = coarse + j1 s1 + j2 s2 + j3 s3.
T_LOGITS = {"half": 0.0, "one": 40.0, "below_one": 13.0, "tiny": -69.0777}
T_K = 50
LEVELS = 4


def _t_job(es2):
    """es2: [users, 4 rows, 256] float32, the second population's e s per user and row."""
    names = list(T_LOGITS)
    U = len(names)
    Pn, Jn = 768, 4 * U
    e = np.ones((Jn, Pn), np.float32)
    es = np.zeros((Jn, Pn), np.float32)
    rows = []
    for u, name in enumerate(names):
        r = np.arange(4 * u, 4 * u + 4)
        rows.append(r.astype(np.int64))
        es[r[0], :256] = np.float32(2.0 * T_LOGITS[name])
        es[r, 256:512] = es2[u]
    items = (512 + np.arange(Jn)).astype(np.int64)      # history POIs lie outside the two populations
    rowmap = np.zeros(Pn, np.int32)
    rowmap[items] = np.arange(Jn, dtype=np.int32)
    indptr = (4 * np.arange(U + 1)).astype(np.int64)
    indices = np.concatenate([items[r] for r in rows]).astype(np.int64)
    return dict(family="threshold", P=Pn, J=Jn, rows=rows, items=items, rowmap=rowmap, indptr=indptr,
                indices=indices, e=e, es=es, et=e, est=es, hi=pb.pack_hi(e, es), widen=None)


T_BLOCKS = [(0, 256, 256), (256, 256, 256)]


@functools.lru_cache(maxsize=None)
def _threshold_tables():
    """The second population found level by level on hi words (upper scores rise with N): returns
    es2 [U, 4, 256] whose last level steps N by less than an fp32 ulp across tau."""
    U = len(T_LOGITS)
    n1 = np.array([2.0 * l for l in T_LOGITS.values()])
    # level 0: coarse values around n1 that hi words hold exactly (8 significant bits), 128 below
    # and 128 above in steps of 2^-7 of |n1| (of 2^-7 where n1 = 0)
    scale = 2.0 ** np.floor(np.log2(np.maximum(np.abs(n1), 1.0)))
    step = scale * 2.0 ** -7
    base = np.round(n1 / step) * step - 128 * step
    es2 = np.zeros((U, 4, 256), np.float32)
    tau = None
    for lev in range(LEVELS):
        sweep = np.arange(256)[None, :] * step[:, None]
        es2[:, lev, :] = ((base[:, None] if lev == 0 else 0.0) + sweep).astype(np.float32)
        dj = bi.DevJob(_t_job(es2))
        if tau is None:   # the first population's k-th lower key: the same at every level
            tau = bi.bound(dj, bi.Lists(U, T_K, 1024), 0.5, blocks=T_BLOCKS[:1])[0][:, T_K - 1].copy()
        upper, _ = intervals("hi", dj, 0.5, T_BLOCKS[1:])
        for u in range(U):
            below = np.flatnonzero((upper[u, 256:512] >> np.uint64(32)) < (tau[u] >> np.uint64(32)))
            assert 0 < below.size < 256, (lev, u, below.size)
            j = below.max()
            assert np.array_equal(below, np.arange(j + 1)), (lev, u, "upper scores do not rise with N")
            if lev < LEVELS - 1:
                es2[u, lev, :] = es2[u, lev, j]      # this level stays at the value just under tau
        step = step / 128.0
    es2.setflags(write=False)
    return es2


@pytest.mark.parametrize("fmt", FORMATS)
def test_survivors_at_the_threshold(fmt):
    es2 = _threshold_tables()
    job = _t_job(es2)
    dj = qi.QJob(job)
    upper, lower = intervals(fmt, dj, 0.5, T_BLOCKS)
    check(fmt, dj, 0.5, T_BLOCKS, T_K, 1024, upper, lower)
    check(fmt, dj, 0.5, T_BLOCKS, 256, 1024, upper, lower)
    lo_keys = _run(fmt, dj, bi.Lists(dj.U, T_K, 1024), 0.5, T_BLOCKS[:1])[0]
    for u, name in enumerate(T_LOGITS):
        ts = pb.split_key(lo_keys[u, T_K - 1])[0][0]
        us = pb.split_key(upper[u, 256:512])[0]
        d = (pb.ord_bits(us).astype(np.int64) - int(pb.ord_bits(ts)[0]))
        print(f"{fmt} {name}: k-th score {ts!r}; second population's upper scores {d.min()} .. {d.max()} ulps "
              f"from it, {np.unique(d).size} distinct")
        if fmt == "hi":   # both sides of tau, a last step of N (under an fp32 ulp of it) apart
            assert d.min() < 0 <= d.max(), (name, d.min(), d.max())
    for u, name in enumerate(T_LOGITS):   # the k-th scores are at 1.0f, 1e-30, 0.5 and just below 1
        ts = float(pb.split_key(lo_keys[u, T_K - 1])[0][0])
        if name == "one":
            assert ts == 1.0, ts
        elif name == "tiny":
            assert 1e-31 < ts < 1e-29, ts
        elif name == "half":
            assert abs(ts - 0.5) < 1e-3, ts
        else:
            assert 1.0 - 1e-5 < ts < 1.0, ts
