"""CPU: the q16 pair-word format (include/nais.h "q16") in numpy: tests/_q16_format.py's reference
quantiser keeps the format's contract, its scales are not vacuous, and the numpy port of the
bounded gather's q16 interval (nais_pairs.hip make_bounds_q16) contains the exact score.

Inputs: the families of tests/_pair_bounds.py (tiny_s, edge and the signed patterns included) and
rows whose values span five decades inside one group of 16 columns.

Scales: q <= (1 + 2^-6) x need (need = the group's max e / 255, max |e*s| / 127 over its valid
columns) wherever need >= 2^-100. Below that the 16-bit scale cannot keep 2^-6 (under 2^-126 its
step is 2^-133) and the quantiser's reciprocal overflows, so the format stores exactly 2^-100 there
-- the contract holds all the same -- and 0 for an all-zero group. The tiny, tiny_s and edge
families live below that floor: their words carry no information (m = 0), which the interval test
sees as "not finite", never as a wrong bound."""
import numpy as np
import pytest

import _pair_bounds as pb
import _q16_format as qf

WIDENS = {"zero": (0.0, 0.0), "x1": (5.65e-3, 1e-3), "limit": (2.0 ** -7, 1e-3)}
LENGTHS = (1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 200, 0)


def _decades(rng, J, P):
    """e and s whose magnitudes span five decades inside every group of 16 columns."""
    e = (10.0 ** rng.uniform(-3, 2, (J, P))).astype(np.float32)
    s = 10.0 ** rng.uniform(-3, 2, (J, P)) * rng.choice([-1.0, 1.0], size=(J, P))
    return e, (e.astype(np.float64) * s).astype(np.float32)


def _tables():
    out = []
    for fam in pb.FAMILIES:
        for pat in pb.PATTERNS:
            job = pb.build_job(fam, 256, 64, (3,), pat, seed=2)
            out.append((f"{fam}/{pat}", job["et"], job["est"]))
    out.append(("decades", *_decades(np.random.default_rng(5), 64, 256)))
    return out


@pytest.mark.parametrize("cols,ld", [(256, 256), (37, 512), (17, 20), (1, 4)])
def test_quantiser_keeps_the_contract_and_tight_scales(cols, ld):
    assert qf.pitch(512) == 1152 and qf.pitch(16) == 128 and qf.pair_offset(512) == 128
    for name, e, p in _tables():
        e, p = e[:, :cols], p[:, :cols]
        blk = qf.quantise(e, p, ld)
        assert blk.shape == (e.shape[0], qf.pitch(ld))
        me, ms, qe, qs = qf.dequantise(blk, ld, cols)
        assert me.min() >= 0 and me.max() <= 255 and ms.min() >= -128 and ms.max() <= 127
        bad = qf.contract_violations(e, p, me, ms, qe, qs)
        assert not bad.any(), (name, cols, int(bad.sum()))
        ex = qf.scale_excess(e, p, blk, ld, cols)
        ex = ex[~np.isnan(ex)]
        assert np.all(ex >= 1.0) and np.all(ex <= qf.TIGHT), (name, cols, float(ex.min()), float(ex.max()))
        # the same from the words alone (what the GPU table test asserts of the kernel): the largest
        # m_e of a finite group above the floor is >= 251, the largest |m_s| >= 125
        g = np.arange(cols) // 16
        for gi in range((cols + 15) // 16):
            c = g == gi
            for m, q, least in ((me, qe, 251), (np.abs(ms), qs, 125)):
                qg = q[:, c][:, 0]
                live = np.isfinite(qg) & (qg > np.float32(qf.SCALE_MIN))
                assert np.all(m[:, c].max(1)[live] >= least), (name, cols, gi, least)
        # the padding is untouched (0xFF) and nothing of it is read back
        ng, off = (cols + 15) // 16, qf.pair_offset(ld)
        assert np.all(blk[:, 4 * ng:off] == 0xFF) and np.all(blk[:, off + 2 * cols:] == 0xFF)


def test_special_groups():
    e = np.ones((4, 32), np.float32)
    p = np.full((4, 32), 0.5, np.float32)
    e[0, :16] = 0.0                   # an all-zero e group
    p[0, :16] = -0.0
    p[1, 3] = np.nan                  # non-finite values make their group's scale non-finite
    e[2, 20] = np.inf
    e[3, :16] = 2.0 ** -120           # below the floor
    me, ms, qe, qs = qf.dequantise(qf.quantise(e, p), 32, 32)
    assert np.all(qe[0, :16] == 0) and np.all(qs[0, :16] == 0) and not me[0, :16].any() and not ms[0, :16].any()
    assert not np.isfinite(qs[1, :16]).any() and np.isfinite(qs[1, 16:]).all() and np.isfinite(qe[1]).all()
    assert not np.isfinite(qe[2, 16:]).any() and np.isfinite(qe[2, :16]).all()
    assert np.all(qe[3, :16] == np.float32(qf.SCALE_MIN)) and not me[3, :16].any()
    assert not qf.contract_violations(e, p, me, ms, qe, qs).any()


@pytest.mark.parametrize("wname", list(WIDENS))
@pytest.mark.parametrize("beta", [0.5, 0.7])
@pytest.mark.parametrize("family", pb.FAMILIES + ("decades",))
def test_port_of_the_q16_bounds_contains_the_exact_score(family, beta, wname):
    """lower <= float64 score of the sequential fp32 sums <= upper for every candidate whose interval
    is finite, at the three widenings; a never-finite family (below the scales' floor) passes by
    having none. The logit ends (after their 2^-19 widening) are held to the float64 logit of the
    fp32 sums with no slack. The score ends are fp32 values of an fp32 sigmoid and bound the fp32
    score the exact gather computes, which lies within the project's TIE_ULPS = 4 of the float64
    score (tests/test_gpu_bound_intervals.py): they are compared with that slack. A candidate
    without a finite interval has nothing to contain: the kernel refines it whatever tau is."""
    widen = WIDENS[wname]
    modes = pb.MODES if widen != (0.0, 0.0) else ("random",)
    patterns = pb.PATTERNS if family != "decades" else ("keep",)
    finite = total = 0
    for pattern in patterns:
        for mode in modes:
            if family == "decades":
                rng = np.random.default_rng(11)
                job = pb.build_job("benign", 256, 256, LENGTHS, "keep", widen=widen, mode=mode, beta=beta)
                e0, p0 = _decades(rng, 256, 256)
                job = dict(job, et=e0, est=p0)
                eta, ds = widen
                sg = rng.choice([-1.0, 1.0], size=e0.shape)
                job["e"] = (e0.astype(np.float64) * (1 + 0.999 * eta * sg)).astype(np.float32)
                s0 = p0.astype(np.float64) / e0
                job["es"] = (job["e"].astype(np.float64) * (s0 - 0.999 * ds * sg)).astype(np.float32)
            else:
                job = pb.build_job(family, 256, 256, LENGTHS, pattern, widen=widen, mode=mode, beta=beta)
            me, ms, qe, qs = qf.dequantise(qf.quantise(job["et"], job["est"]), 256, 256)
            eta, ds = widen
            for rows in job["rows"]:
                if len(rows) == 0:
                    continue
                S32, N32 = pb.seq_sums(job["e"][rows], job["es"][rows])
                ref = pb.ref_score(S32, N32, beta)
                S, N, Qe, Qs = qf.seq_sums_q16(me[rows], ms[rows], qe[rows], qs[rows])
                lo, up, ok = qf.interval_q16(S, N, Qe, Qs, len(rows), beta, eta, ds)
                cand = np.ones(256, bool)
                cand[job["items"][rows]] = False
                ok = ok & cand
                total += int(cand.sum())
                finite += int(ok.sum())
                assert not np.isnan(ref[ok]).any(), (family, pattern, mode)
                # ... and below fp32's normal range the fp32 sigmoid itself returns 0 (expf overflows)
                slack = 4 * np.spacing(np.abs(ref[ok]).astype(np.float32)).astype(np.float64) + 2.0 ** -126
                assert np.all(lo[ok] <= ref[ok] + slack), (family, pattern, mode, len(rows))
                assert np.all(up[ok] >= ref[ok] - slack), (family, pattern, mode, len(rows))
                # the logit ends against the float64 logit of the same fp32 sums: no slack
                ll, lu, _ = qf.interval_q16(S, N, Qe, Qs, len(rows), beta, eta, ds, logits=True)
                with np.errstate(all="ignore"):
                    S64, N64 = S32.astype(np.float64), N32.astype(np.float64)
                    logit = N64 / (np.sqrt(S64) if beta == 0.5 else S64 ** float(np.float32(beta)))
                assert np.all(ll[ok] <= logit[ok]) and np.all(logit[ok] <= lu[ok]), (family, pattern, mode, len(rows))
    print(f"{family} beta {beta} widen {wname}: finite {finite} of {total}")
    # not vacuous: a candidate has no finite interval when every m_e of its history is 0 (e below
    # 1 / 255 of its group's largest). Never around 17 (e within 5 % of 1); for a ~ N(., 1) that
    # takes a value 5.5 below the group's largest, less than 1e-4 of the entries.
    if family == "around17":
        assert finite == total
    if family in ("benign", "cancelling"):
        assert finite >= 0.99 * total
