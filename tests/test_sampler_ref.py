"""The host model of the batch sampler (tests/_sampler_ref.py): the permutation is a bijection and
the batches drawn through it are uniform. The GPU tests (tests/test_gpu_batch_builders.py) show
that the kernels compute exactly this model, so the sampler's distribution rests on this file.

The seeds are fixed, so every statistic below is deterministic; the bound is the 99.9 % quantile
of the chi-square distribution with (cells - 1) degrees of freedom."""
import numpy as np
import pytest
from scipy.stats import chi2

import _sampler_ref as sr

SIZES = [2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097,
         5003, 65535, 65536, 65537, 2 ** 20, 2 ** 20 + 1]
SEEDS = [0, 1, 0xDEADBEEF, 0xFFFFFFFF]

P, POS, TRIALS = 64, np.array([3, 10, 11, 40, 41, 63]), 3000
FREE = np.setdiff1d(np.arange(P), POS)


def test_mix32_and_half_bits_known_values():
    assert int(sr.mix32(0)) == 0
    x = 1                                   # the C expression on Python integers

    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    assert int(sr.mix32(1)) == x
    assert np.array_equal(sr.mix32(np.array([0, 1])), [0, x])
    # k = bit_length(m - 1): 2 -> 1 bit -> 1; 3, 4 -> 2 -> 1; 5 -> 3 -> 2; 16 -> 4 -> 2; 17 -> 5 -> 3
    assert [sr.half_bits(m) for m in (2, 3, 4, 5, 16, 17, 1024, 1025, 2 ** 31)] == [1, 1, 1, 2, 2, 3, 5, 6, 16]


def test_permute_degenerate():
    assert np.array_equal(sr.permute(np.arange(3), 1, 5), [0, 0, 0])
    assert np.array_equal(sr.permute(np.arange(3), 0, 5), [0, 0, 0])


@pytest.mark.parametrize("s", SEEDS)
def test_permute_is_a_bijection(s):
    walk = [0]
    for m in SIZES:
        out = sr.permute(np.arange(m), m, s, walk=walk)
        assert out.min() >= 0 and out.max() < m
        assert np.array_equal(np.bincount(out, minlength=m), np.ones(m, np.int64)), m
    # longest cycle walk measured: 46, 57, 55, 50 applications for the four seeds (the domain
    # 4^hb is up to four times m, so a walk of w has probability ~(3/4)^w); the bound only
    # reports a key that degenerates
    print(f"seed {s:#x}: longest cycle walk {walk[0]}")
    assert walk[0] <= 200


def _chi2(counts):
    e = counts.sum() / len(counts)
    return float(((counts - e) ** 2 / e).sum())


def test_bpr_negatives_uniform():
    cnt = np.zeros(P)
    for seed in range(TRIALS):
        u, i, j = sr.bpr_batch(POS, 0, P, seed)
        assert np.array_equal(i, POS) and len(set(j.tolist())) == len(POS)
        np.add.at(cnt, j, 1)
    assert cnt[POS].sum() == 0 and cnt.sum() == TRIALS * len(POS)
    stat, q = _chi2(cnt[FREE]), chi2.ppf(0.999, len(FREE) - 1)
    print(f"BPR negatives: chi-square {stat:.1f}, 99.9 % quantile {q:.1f}")   # measured 76.2 < 95.8
    assert stat < q


def test_nais_negatives_and_first_history_position_uniform():
    cnt, first = np.zeros(P), np.zeros(len(POS))
    for seed in range(TRIALS):
        hist, tgt, lab = sr.nais_batch(POS, P, 4, seed)
        assert sorted(hist.tolist()) == POS.tolist()
        rows = tgt.reshape(len(POS), 5)
        assert np.array_equal(rows[:, 0], hist)
        neg = rows[:, 1:].reshape(-1)
        assert len(set(neg.tolist())) == len(neg)
        np.add.at(cnt, neg, 1)
        first[np.searchsorted(POS, hist[0])] += 1
    assert cnt[POS].sum() == 0 and cnt.sum() == TRIALS * len(POS) * 4
    # a batch draws 24 of the 58 free POIs WITHOUT replacement, so a cell's variance is the
    # multinomial's times (1 - 24/58): the statistic sits below the chi-square it is held to
    stat, q = _chi2(cnt[FREE]), chi2.ppf(0.999, len(FREE) - 1)
    print(f"NAIS negatives: chi-square {stat:.1f}, 99.9 % quantile {q:.1f}")   # measured 24.0 < 95.8
    assert stat < q
    stat1, q1 = _chi2(first), chi2.ppf(0.999, len(POS) - 1)
    print(f"NAIS first history position: chi-square {stat1:.1f}, 99.9 % quantile {q1:.1f}")   # 5.8 < 20.5
    assert stat1 < q1


def test_batches_depend_on_the_whole_seed_and_the_user():
    row = np.arange(0, 100, 2)
    a = sr.nais_batch(row, 3000, 4, 5)
    b = sr.nais_batch(row, 3000, 4, 5 + (1 << 32))
    assert np.array_equal(a[0], b[0])              # the history order takes the low word only
    assert not np.array_equal(a[1], b[1])          # the negatives take both
    ja = sr.bpr_batch(row, 3, 3000, 5)[2]
    assert np.array_equal(ja, sr.bpr_batch(row, 3, 3000, 5)[2])
    assert not np.array_equal(ja, sr.bpr_batch(row, 4, 3000, 5)[2])
    assert not np.array_equal(ja, sr.bpr_batch(row, 3, 3000, 5 + (1 << 32))[2])
