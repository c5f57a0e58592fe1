"""Numpy helpers for the tests of the bounded gather's score intervals (tests/test_gpu_bound_intervals.py,
tests/test_pair_bounds_reference.py). No GPU and no import of the package: the key of include/nais.h,
the split16 hi word, the exact gather's sequential fp32 sums, a float64 score, the score interval
that the hi words' contract alone allows (no fp32-rounding terms), and hand-built pair tables.

A job is a dict: P columns (POI ids 0 .. P-1), J table rows (the distinct history POIs `items`,
rowmap[poi] = row), a CSR of histories (`indptr`, `indices`: POI ids, ascending per user), and the
[J, P] float32 tables
  e, es      the exact pair values (what the exact gather and the refine sum),
  et, est    the tabled pair the hi words truncate (the same arrays unless the job is widened),
  hi         pack_hi(et, est).
block_tables() cuts the device layout of one column block out of a job."""
from __future__ import annotations

import numpy as np

NAN_BITS = np.uint32(0x7FC00000)
FAMILIES = ("benign", "cancelling", "around17", "tiny", "tiny_s", "edge", "huge", "zero")
# low 16 bits of e and es: all zero, all one, random, and the two corners of the score interval --
# "signed_up": e at its truncation, es at the far end where positive and at its truncation where
# negative (S lowest, N highest), "signed_down" the mirror image
PATTERNS = ("zeros", "ones", "random", "signed_up", "signed_down")
# widening: every d and t up, every one down, random signs, and d by the sign of the term
# ("signed_up": e up where e s > 0 and down where e s < 0, so N moves by eta A; t up) and its mirror
MODES = ("up", "down", "random", "signed_up", "signed_down")


# ---- keys (include/nais.h: ordered(score) << 32 | (0xFFFFFFFF - poi), NaN above +inf) ----------
def ord_bits(score):
    s = np.atleast_1d(np.asarray(score, dtype=np.float32))
    u = np.where(np.isnan(s), NAN_BITS, s.view(np.uint32))
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def ord_key(score_f32, poi):
    o = ord_bits(score_f32).astype(np.uint64)
    p = (np.uint64(0xFFFFFFFF) - np.atleast_1d(np.asarray(poi)).astype(np.uint64))
    return (o << np.uint64(32)) | p


def split_key(key):
    """key -> (float32 score, int64 poi)."""
    key = np.atleast_1d(np.asarray(key)).astype(np.uint64)
    o = (key >> np.uint64(32)).astype(np.uint32)
    bits = np.where(o & np.uint32(0x80000000), o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32)
    poi = (np.uint64(0xFFFFFFFF) - (key & np.uint64(0xFFFFFFFF))).astype(np.int64)
    return bits.view(np.float32), poi


# ---- the split16 word and its two truncated values -----------------------------------------------
def pack_hi(e, es):
    """(top 16 bits of es) << 16 | (top 16 bits of e)."""
    eb = np.ascontiguousarray(e, dtype=np.float32).view(np.uint32)
    sb = np.ascontiguousarray(es, dtype=np.float32).view(np.uint32)
    return (sb & np.uint32(0xFFFF0000)) | (eb >> np.uint32(16))


def hi_values(hi):
    """(e^, es~) of hi words as float32: e^ = e truncated to 16 bits; es~ = the word read as a float
    (the top 16 bits of e*s followed by those of e), as the bounded gather sums them."""
    hi = np.ascontiguousarray(hi, dtype=np.uint32)
    return (hi << np.uint32(16)).view(np.float32), hi.view(np.float32)


# ---- the exact gather in numpy -----------------------------------------------------------------
def seq_sums(e_rows, es_rows):
    """fp32 sums over the history rows [h, C] in the given (CSR) order: one row-vector add per
    entry, np.float32 accumulators."""
    e_rows = np.asarray(e_rows, dtype=np.float32)
    es_rows = np.asarray(es_rows, dtype=np.float32)
    S = np.zeros(e_rows.shape[1:], np.float32)
    N = np.zeros(e_rows.shape[1:], np.float32)
    with np.errstate(all="ignore"):
        for j in range(e_rows.shape[0]):
            S = (S + e_rows[j]).astype(np.float32)
            N = (N + es_rows[j]).astype(np.float32)
    return S, N


def _sigmoid64(l):
    with np.errstate(all="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(l, np.float64)))


def ref_score(S32, N32, beta, empty=False):
    """sigmoid(N / S**beta) in float64 from the fp32 sums (NaN where the logit is: 0 / 0, inf / inf,
    a NaN sum); an empty history scores sigmoid(0). beta is rounded to float32 first, as the C-ABI
    takes it: at S ~ 2^-115 the difference between 0.7 and float32(0.7) is 16 ulps of S^beta."""
    S = np.asarray(S32, np.float64)
    N = np.asarray(N32, np.float64)
    if empty:
        return np.full(S.shape, 0.5)
    with np.errstate(all="ignore"):   # beta as the kernels get it: a float32
        return _sigmoid64(N / (np.sqrt(S) if beta == 0.5 else S ** float(np.float32(beta))))


def ulps32(got_f32, want_f64):
    """|got - want| in units of the fp32 spacing at |want| (inf where exactly one is NaN)."""
    got = np.asarray(got_f32, np.float64)
    want = np.asarray(want_f64, np.float64)
    with np.errstate(all="ignore"):
        sp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        d = np.abs(got - want) / sp
    both = np.isnan(got) & np.isnan(want)
    one = np.isnan(got) ^ np.isnan(want)
    return np.where(both, 0.0, np.where(one, np.inf, d))


# ---- the interval the contract alone allows ------------------------------------------------------
def ideal_interval(hi_rows, beta, eta=0.0, ds=0.0):
    """(lo, hi) score bounds in float64 from the hi words [h, C] of a history, by the contract alone:
      S in [S^ (1 - eta), S^ (1 + 2^-7)(1 + eta)],
      |N - N^| <= (2^-7 + 1.02 eta) A^ + S^ (1 + 2^-7)(1 + eta) ds,
    S^, N^, A^ the float64 sums of e^, es~, |es~|, evaluated at the corners the kernel takes (the
    sign of the N bound picks the S end). NaN where S^ is 0 or a sum is not finite; an empty
    history gives 0.5 on both sides."""
    eh, st = hi_values(hi_rows)
    beta = float(np.float32(beta))
    C = eh.shape[1:]
    if eh.shape[0] == 0:
        return np.full(C, 0.5), np.full(C, 0.5)
    with np.errstate(all="ignore"):
        S = eh.astype(np.float64).sum(0)
        N = st.astype(np.float64).sum(0)
        A = np.abs(st.astype(np.float64)).sum(0)
        slo = S * (1.0 - eta)
        shi = S * (1.0 + 2.0 ** -7) * (1.0 + eta)
        rn = (2.0 ** -7 + 1.02 * eta) * A + shi * ds
        nlo, nhi = N - rn, N + rn
        dlo, dhi = slo ** beta, shi ** beta
        up = np.where(nhi >= 0, nhi / dlo, nhi / dhi)
        dn = np.where(nlo >= 0, nlo / dhi, nlo / dlo)
        ok = (slo > 0) & np.isfinite(shi) & np.isfinite(nlo) & np.isfinite(nhi)
        return np.where(ok, _sigmoid64(dn), np.nan), np.where(ok, _sigmoid64(up), np.nan)


# ---- hand-built tables ---------------------------------------------------------------------------
def low_bits(x, pattern, rng):
    """x (float32) with the low 16 bits of every word forced: zeros (x equals its truncation), ones
    (the far end of the truncation) or random; "keep" leaves x as it is. The exponent field is
    untouched: finite stays finite."""
    if pattern == "keep":
        return np.ascontiguousarray(x, dtype=np.float32)
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    if pattern == "ones":
        b = b | np.uint32(0xFFFF)
    elif pattern == "random":
        b = b | rng.integers(0, 1 << 16, size=b.shape, dtype=np.uint32)
    elif pattern != "zeros":
        raise ValueError(pattern)
    return b.view(np.float32)


def family_values(family, rng, J, P, shuffle=False, spread=8e-5, beta=0.5):
    """(e float32 [J, P], s float64 [J, P]) of one input family."""
    with np.errstate(all="ignore"):
        if family == "benign":            # a ~ N(0, 1), s > 0
            e = np.exp(rng.normal(0, 1, (J, P)))
            s = rng.uniform(0.02, 0.5, (J, P))
        elif family == "cancelling":      # s ~ N(0, 1); every 4th column sums +-s pairs to N ~ 0
            # a ~ N(-3, 1): the logit's deviation is sqrt(E e^2 / E e) = e^(-3/4) ~ 0.5 at every h.
            # An fp32 logit is known to 2^-24 |l| at best, which exp turns into |l| half-ulps of a
            # score below 1/2: only for |l| of a few can any fp32 gather sit within TIE_ULPS of the
            # float64 reference, so the family keeps its logits there (A / |N| is what it is about).
            e = np.exp(rng.normal(-3, 1, (J, P)))
            s = rng.normal(0, 1, (J, P))
            c = np.arange(0, P, 4)
            e[:, c] = np.exp(rng.normal(-3, 1, c.size))[None, :]
            s[:, c] = rng.uniform(0.1, 1.0, c.size)[None, :] * np.where(np.arange(J) % 2 == 0, 1.0, -1.0)[:, None]
        elif family == "around17":        # h = 16, e ~ 1: logit ~ 16^(1 - beta) s, 14 .. 20 in steps of 6 / P
            l = np.linspace(14.0, 20.0, P)
            if shuffle:
                l = rng.permutation(l)
            e = np.exp(rng.normal(0, 0.01, (J, P)))
            s = l[None, :] / 16.0 ** (1.0 - beta) * (1.0 + rng.uniform(-1e-3, 1e-3, (J, P)))
        elif family == "tiny":            # e down into the denormals (and to 0)
            e = np.exp(rng.uniform(-104.0, -84.0, (J, P)))
            s = rng.normal(0, 1, (J, P))
        elif family == "tiny_s":          # subnormal e whose 16-bit truncation loses up to all of it
            # (e in 2^-133.5 .. 2^-126: e - e^ < 2^-133 is no longer 2^-7 of e^), with s ~ 2^62 (at
            # beta = 0.5) so that the logit ~ s e^(1 - beta) is of order 1 at every beta and the score shows a wrong S bound: the family
            # that needs the absolute h 2^-126 term of the S interval
            e = np.exp(rng.uniform(-92.5, -87.4, (J, P)))
            s = 2.0 ** (133 * (1 - beta) - 4.5) * rng.uniform(0.5, 2.0, (J, P)) * rng.choice([-1.0, 1.0], size=(J, P))
        elif family == "edge":            # the truncation margins used up: e and e s powers of two
            # (the kept mantissa bits all 0, so the "ones" pattern puts both 2^-7 above their
            # truncation) and e ~ 2^-120, whose top bits are 1.4 % of the low half of es~. What is
            # left of the 2^-7 A^ term is then of the size of the rounding terms (4 g) and below eta.
            e = 2.0 ** rng.integers(-120, -117, (J, P)).astype(np.float64)
            q = int(round(-119 * beta))      # e s ~ S^beta: logits of order 1
            s = 2.0 ** rng.integers(q - 1, q + 1, (J, P)).astype(np.float64) / e * rng.choice([1.0, 1.0, 1.0, -1.0], size=(J, P))
        elif family == "huge":            # sums overflow for long histories
            e = np.exp(rng.uniform(80.0, 88.7, (J, P)))
            s = 1e-3 * rng.normal(0, 1, (J, P))
        elif family == "zero":
            e = np.zeros((J, P))
            s = rng.normal(0, 1, (J, P))
        elif family == "clustered":       # every score within 1e-4 of 0.5 (the reference's init)
            e = np.exp(rng.normal(0, 0.01, (J, P)))
            s = spread * rng.normal(0, 1, (J, P))
        elif family == "rising":          # exact scores rise with the column: 0.1 % of logit a column
            e = np.repeat(np.exp(rng.normal(0, 0.05, (J, 1))), P, axis=1)
            s = np.repeat(0.02 * np.exp(1e-3 * np.arange(P))[None, :], J, axis=0)
        else:
            raise ValueError(family)
        return e.astype(np.float32), s.astype(np.float64)


def make_histories(rng, J, lengths, paired=False):
    """Row sets (ascending) of the given lengths; paired: rows (2i, 2i + 1) together (an odd
    length takes one more single row)."""
    out = []
    for h in lengths:
        if paired:
            p = rng.permutation(J // 2)
            rows = np.concatenate([2 * p[:h // 2], 2 * p[:h // 2] + 1, 2 * p[h // 2:h // 2 + h % 2]])
        else:
            rows = rng.permutation(J)[:h]
        out.append(np.sort(rows).astype(np.int64))
    return out


A_LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 128, 129, 200, 0)


def family_lengths(family, lengths):
    return tuple(16 if h else 0 for h in lengths) if family == "around17" else tuple(lengths)


def build_job(family, P, J, lengths, pattern="random", seed=0, widen=None, mode="random",
              item_stride=1, item_first=0, shuffle=False, spread=8e-5, beta=0.5):
    """The job of one family (beta: the around-17 family aims its logits at it). widen = (eta, ds)
    or None. With widening the hi words truncate the tabled pair (e~, p~ = e~ s~); the exact tables
    hold e = fp32(e~ (1 + d)), |d| <= 0.999 eta, and es = fp32(e (s~ + t)), |t| <= 0.999 ds: mode "up" (d = +0.999 eta, t = +0.999 ds: es up),
    "down" (both negative) or random signs; s~ = p~ / e~ is a real number (float64), so e (s~ + t)
    is rounded once; "signed_up" / "signed_down" take d by the sign of the term. Where fp32 rounding alone would carry e out of e~ [1 - eta, 1 + eta] (a
    denormal e~) the entry keeps d = 0."""
    rng = np.random.default_rng([seed, FAMILY_SEED[family], (PATTERNS[:3] + ("keep",) + PATTERNS[3:]).index(pattern)])
    e0, s0 = family_values(family, rng, J, P, shuffle=shuffle, spread=spread, beta=beta)
    pe = {"signed_up": "zeros", "signed_down": "ones"}.get(pattern, pattern)
    et = low_bits(e0, pe, rng)
    with np.errstate(all="ignore"):
        est = (et.astype(np.float64) * s0).astype(np.float32)
        if pattern in ("signed_up", "signed_down"):   # magnitude up <-> value up only where positive
            far = (est > 0) == (pattern == "signed_up")
            est = np.where(far, low_bits(est, "ones", rng), low_bits(est, "zeros", rng))
        else:
            est = low_bits(est, pattern, rng)
        eta, ds = (0.0, 0.0) if widen is None else (float(widen[0]), float(widen[1]))
        if eta == 0.0 and ds == 0.0:
            e, es = et, est
        else:
            st = np.where(et > 0, est.astype(np.float64) / et.astype(np.float64), s0)   # p~ = e~ s~
            if mode == "random":
                sg_e = rng.choice([-1.0, 1.0], size=et.shape)
                sg_s = rng.choice([-1.0, 1.0], size=et.shape)
            elif mode in ("signed_up", "signed_down"):
                sg_s = np.full(et.shape, 1.0 if mode == "signed_up" else -1.0)
                sg_e = np.where(est < 0, -1.0, 1.0) * sg_s
            else:
                sg_e = sg_s = np.full(et.shape, 1.0 if mode == "up" else -1.0)
            e = (et.astype(np.float64) * (1.0 + 0.999 * eta * sg_e)).astype(np.float32)
            e = np.where(np.abs(e.astype(np.float64) - et) <= eta * et.astype(np.float64), e, et)
            es = (e.astype(np.float64) * (st + 0.999 * ds * sg_s)).astype(np.float32)   # one rounding
    lengths = family_lengths(family, lengths)
    hist = make_histories(rng, J, lengths, paired=(family == "cancelling"))
    items = (item_first + item_stride * np.arange(J)).astype(np.int64)
    assert items[-1] < P
    rowmap = np.zeros(P, np.int32)
    rowmap[items] = np.arange(J, dtype=np.int32)
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in hist])]).astype(np.int64)
    indices = (np.concatenate([items[r] for r in hist]) if indptr[-1] else np.zeros(0)).astype(np.int64)
    return dict(family=family, P=P, J=J, rows=hist, items=items, rowmap=rowmap, indptr=indptr,
                indices=indices, e=e, es=es, et=et, est=est, hi=pack_hi(et, est), widen=widen)


FAMILY_SEED = {f: i for i, f in enumerate(("benign", "cancelling", "around17", "tiny", "huge", "zero",
                                            "clustered", "rising", "tiny_s", "edge"))}


def block_tables(job, col0, cols, ld):
    """The device layout of columns [col0, col0 + cols): e, es float32 [J, ld], the interleaved ex
    [J, 2 ld] and hi [J, ld] as uint32. The pitch padding holds NaN bits: a kernel that summed a
    padding column would show it."""
    J = job["J"]
    sl = slice(col0, col0 + cols)
    e = np.full((J, ld), NAN_BITS, np.uint32)
    es = e.copy()
    hi = e.copy()
    e[:, :cols] = job["e"][:, sl].view(np.uint32)
    es[:, :cols] = job["es"][:, sl].view(np.uint32)
    hi[:, :cols] = job["hi"][:, sl]
    ex = np.empty((J, 2 * ld), np.uint32)
    ex[:, 0::2] = e
    ex[:, 1::2] = es
    return e.view(np.float32), es.view(np.float32), ex, hi


def exact_reference(job, beta):
    """(score float64 [U, P], candidate mask [U, P]) from seq_sums + ref_score; history columns are
    no candidates."""
    U = len(job["rows"])
    sc = np.empty((U, job["P"]))
    cand = np.ones((U, job["P"]), bool)
    for u, rows in enumerate(job["rows"]):
        S, N = seq_sums(job["e"][rows], job["es"][rows])
        sc[u] = ref_score(S, N, beta, empty=len(rows) == 0)
        cand[u, job["items"][rows]] = False
    return sc, cand
