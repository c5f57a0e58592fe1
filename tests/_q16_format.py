"""Numpy reference of the q16 pair-word format (include/nais.h, "q16"): a quantiser, a dequantiser,
the format's contract, and a port of the bounded gather's q16 sums and score interval
(bound_rows_q16 / make_bounds_q16 / upper_score / lower_score in nais_pairs.hip). No GPU and no
import of the package. Used by tests/test_q16_format.py and the GPU tests of the q16 kernels.

A block is a uint8 array [rows, pitch]: per row ceil(ld / 16) scale words (uint32 little endian:
q_s in bits 31..16, q_e in bits 15..0, each the top 16 bits of a non-negative fp32), then ld pair
words (uint16: low byte m_e, high byte m_s + 128). The padding holds 0xFF bytes here (NaN scales,
m = 255 / 127): a kernel that summed a padding column would show it."""
from __future__ import annotations

import numpy as np

GROUP = 16
SLACK = 2.0 ** -14            # of the scale, per value (the quantiser's reciprocal and rounding)
SCALE_MIN = 2.0 ** -100       # the smallest non-zero scale
SCALE_MIN_BITS = np.uint32(0x0D800000)
TIGHT = 1.0 + 2.0 ** -6       # scale <= TIGHT x its group's need
C255 = np.float32((1.0 + 2.0 ** -7) * (1.0 + 2.0 ** -13) / 255.0)
C127 = np.float32((1.0 + 2.0 ** -7) * (1.0 + 2.0 ** -13) / 127.0)


def pitch(ld):
    return (4 * ((ld + GROUP - 1) // GROUP) + 2 * ld + 127) // 128 * 128


def pair_offset(ld):
    return 4 * ((ld + GROUP - 1) // GROUP)


def _group_max_bits(x, cols):
    """uint32 [rows, groups]: the largest |x| bit pattern per group of 16 columns over the first
    `cols` columns (unsigned order: NaN above infinity above every finite value)."""
    rows = x.shape[0]
    ng = (cols + GROUP - 1) // GROUP
    b = np.zeros((rows, ng * GROUP), np.uint32)
    b[:, :cols] = np.ascontiguousarray(x[:, :cols], dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    return b.reshape(rows, ng, GROUP).max(2)


def scale_bits(max_bits, c):
    """The scale (fp32 bits, low 16 zero) of groups whose largest value has the bits max_bits."""
    with np.errstate(all="ignore"):
        q = (max_bits.view(np.float32) * c).astype(np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    q = np.maximum(q, SCALE_MIN_BITS)
    return np.where(max_bits == 0, np.uint32(0), q).astype(np.uint32)


def _mantissa(x, qbits, offset):
    """trunc(x / q + offset) in fp32 as the kernel forms it (reciprocal, one fma), clamped to 0..255."""
    with np.errstate(all="ignore"):
        r = np.where(qbits == 0, np.float32(0), np.float32(1) / qbits.view(np.float32)).astype(np.float32)
        u = (x.astype(np.float64) * r.astype(np.float64) + offset).astype(np.float32)
    u = np.where(np.isnan(u), np.float32(0), np.clip(u, 0, 255))
    return u.astype(np.uint32)   # truncation


def quantise(e, p, ld=None):
    """(e, p) float32 [rows, cols] -> q16 block uint8 [rows, pitch(ld)] (ld defaults to cols)."""
    e = np.ascontiguousarray(e, dtype=np.float32)
    p = np.ascontiguousarray(p, dtype=np.float32)
    rows, cols = e.shape
    ld = cols if ld is None else ld
    assert ld >= cols
    qe = scale_bits(_group_max_bits(e, cols), C255)
    qs = scale_bits(_group_max_bits(p, cols), C127)
    col_group = np.arange(cols) // GROUP
    me = _mantissa(e, qe[:, col_group], 0.0)
    ms = _mantissa(p, qs[:, col_group], 128.0)
    blk = np.full((rows, pitch(ld)), 0xFF, np.uint8)
    sw = (qs & np.uint32(0xFFFF0000)) | (qe >> np.uint32(16))
    blk[:, :4 * sw.shape[1]] = sw.astype("<u4").view(np.uint8).reshape(rows, -1)
    pw = (me | (ms << np.uint32(8))).astype("<u2")
    off = pair_offset(ld)
    blk[:, off:off + 2 * cols] = pw.view(np.uint8).reshape(rows, -1)
    return blk


def dequantise(blk, ld, cols):
    """block -> (m_e, m_s int32 [rows, cols], q_e, q_s float32 [rows, cols] (the column's group's))."""
    rows = blk.shape[0]
    assert blk.shape[1] == pitch(ld)
    ng = (cols + GROUP - 1) // GROUP
    sw = np.ascontiguousarray(blk[:, :4 * ng]).view("<u4").astype(np.uint32).reshape(rows, ng)
    off = pair_offset(ld)
    pw = np.ascontiguousarray(blk[:, off:off + 2 * cols]).view("<u2").astype(np.int32).reshape(rows, cols)
    g = np.arange(cols) // GROUP
    qe = (sw << np.uint32(16)).view(np.float32)[:, g]
    qs = (sw & np.uint32(0xFFFF0000)).view(np.float32)[:, g]
    return pw & 0xFF, (pw >> 8) - 128, qe, qs


def contract_violations(e, p, me, ms, qe, qs):
    """Boolean [rows, cols]: pairs outside (m - 2^-14) q <= value < (m + 1 + 2^-14) q, for either
    value, in float64 (exact here: 9 x 8 significant bits). Groups with a non-finite scale promise
    nothing and are skipped."""
    e64, p64 = np.asarray(e, np.float64), np.asarray(p, np.float64)
    with np.errstate(all="ignore"):
        qe64, qs64 = qe.astype(np.float64), qs.astype(np.float64)
        bad_e = ~(((me - SLACK) * qe64 <= e64) & (e64 < (me + 1 + SLACK) * qe64))
        bad_s = ~(((ms - SLACK) * qs64 <= p64) & (p64 < (ms + 1 + SLACK) * qs64))
        # scale 0: the all-zero group, words 0 / 128
        bad_e = np.where(qe64 == 0, (e64 != 0) | (me != 0), bad_e)
        bad_s = np.where(qs64 == 0, (p64 != 0) | (ms != 0), bad_s)
    return (bad_e & np.isfinite(qe)) | (bad_s & np.isfinite(qs))


def scale_excess(e, p, blk, ld, cols):
    """Per (row, group) and value: scale / need, need = max / 255 or max |.| / 127 over the group's
    valid columns, as float64 [2, rows, groups]; NaN where the rule does not apply (an all-zero or
    non-finite group). A need below SCALE_MIN must give exactly SCALE_MIN: reported as 1.0 when it
    does and inf when it does not."""
    rows = blk.shape[0]
    ng = (cols + GROUP - 1) // GROUP
    sw = np.ascontiguousarray(blk[:, :4 * ng]).view("<u4").astype(np.uint32).reshape(rows, ng)
    out = []
    for x, q, div in ((e, (sw << np.uint32(16)).view(np.float32), 255.0),
                      (p, (sw & np.uint32(0xFFFF0000)).view(np.float32), 127.0)):
        mb = _group_max_bits(np.asarray(x, np.float32), cols)
        with np.errstate(all="ignore"):
            need = mb.view(np.float32).astype(np.float64) / div
            ratio = q.astype(np.float64) / need
        ratio = np.where(need < SCALE_MIN, np.where(q == np.float32(SCALE_MIN), 1.0, np.inf), ratio)
        ratio = np.where(mb == 0, np.where(q == 0, np.nan, np.inf), ratio)
        ratio = np.where(mb >= np.uint32(0x7F800000), np.where(np.isfinite(q), np.inf, np.nan), ratio)
        out.append(ratio)
    return np.stack(out)


# ---- the gather's sums and interval, ported ------------------------------------------------------
def seq_sums_q16(me, ms, qe, qs):
    """The fp32 sums of bound_rows_q16 over history rows [h, C] in order: S^ = sum m_e q_e, N' = sum
    (m_s + 128) q_s (one fma each: exact product, one rounding), Qe, Qs; returns (S^, N^ = N' - 128
    Qs as one fma, Qe, Qs)."""
    C = me.shape[1:]
    S, N, Qe, Qs = (np.zeros(C, np.float32) for _ in range(4))
    with np.errstate(all="ignore"):
        for j in range(me.shape[0]):
            S = (S.astype(np.float64) + me[j] * qe[j].astype(np.float64)).astype(np.float32)
            N = (N.astype(np.float64) + (ms[j] + 128) * qs[j].astype(np.float64)).astype(np.float32)
            Qe = (Qe + qe[j]).astype(np.float32)
            Qs = (Qs + qs[j]).astype(np.float32)
        N = (N.astype(np.float64) - 128.0 * Qs.astype(np.float64)).astype(np.float32)
    return S, N, Qe, Qs


def _sigmoid32(l):
    with np.errstate(all="ignore"):
        return (np.float32(1) / (np.float32(1) + np.exp(-l.astype(np.float32)).astype(np.float32))).astype(np.float32)


def interval_q16(S, N, Qe, Qs, h, beta, eta=0.0, ds=0.0, logits=False):
    """(lower score, upper score, ok) float32 per candidate: make_bounds_q16 / lower_score /
    upper_score evaluated in fp32 as the kernel does (libm's expf / powf stand in for the device's:
    the 2^-19 logit and 2^-20 score widenings are there for them). `logits`: the two logit ends
    (after their 2^-19 widening) instead of the scores."""
    f = np.float32
    eta, ds = f(eta), f(ds)
    eta2 = f(eta * f(1.02) + f(2.0 ** -21)) if eta > 0 else f(0)
    g = f(f(h) * f(2.0 ** -23) + f(2.0 ** -20))
    tiny = f(f(h) * f(2.0 ** -126))
    with np.errstate(all="ignore"):
        A = f(128.0 * (1 + 2.0 ** -10)) * Qs
        su = S + f(1 + 2.0 ** -13) * Qe
        slo = (S - f(2.0 ** -13) * Qe) * (f(1) - f(3) * g) * (f(1) - eta)
        shi = su * (f(1) + f(3) * g) * (f(1) + eta) + tiny
        rn = (f(4) * g + eta2) * A + (tiny + su * f(1 + 2.0 ** -7) * (f(1) + eta) * ds)
        nlo = N - f(512) * g * Qs - rn
        nhi = N + (f(1) + f(512) * g) * Qs + rn
        if beta == 0.5:
            dlo, dhi = np.sqrt(slo), np.sqrt(shi)
        else:
            p0, p1 = np.power(slo, f(beta)), np.power(shi, f(beta))
            dlo, dhi = np.minimum(p0, p1), np.maximum(p0, p1)
        ok = (slo > 0) & (dlo > 0) & np.isfinite(dhi) & np.isfinite(nlo) & np.isfinite(nhi)
        lu = np.where(nhi >= 0, nhi / dlo, nhi / dhi).astype(f)
        lu = lu + np.abs(lu) * f(2.0 ** -19)
        up = np.minimum(_sigmoid32(lu) * f(1 + 2.0 ** -20), f(1))
        ll = np.where(nlo >= 0, nlo / dhi, nlo / dlo).astype(f)
        ll = ll - np.abs(ll) * f(2.0 ** -19)
        if logits:
            return ll.astype(f), lu.astype(f), ok
        lo = np.where(ll >= 17, f(1), _sigmoid32(ll) * f(1 - 2.0 ** -20))
    return lo.astype(f), up.astype(f), ok
