"""Host model of the device-side batch sampler: csrc/nais_sampler.h (mix32, the 8-round Feistel
network, cycle walking) and the seed derivations and slot layout of make_batch_kernel
(csrc/nais_train.hip, also the id half of nais_geoie_make_train_batch) and bpr_make_batch_kernel
(csrc/nais_bpr_train.hip). Integer-exact: numpy uint64 masked to 32 bits, so the kernels can be
held to the exact batch and not only to its properties. Test infrastructure only.
"""
from __future__ import annotations

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
GOLD = 0x9E3779B9


def _u(x):
    return np.asarray(x, dtype=np.uint64) & M32


def mix32(x):
    """nais_sampler.h mix32 on uint32 values held in uint64 (scalar or array)."""
    x = _u(x)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    x = x ^ (x >> np.uint64(16))
    return x


def half_bits(m):
    """Half the bits of the smallest power of two >= m (m >= 2), rounded up."""
    k = int(m - 1).bit_length()
    return (k + 1) >> 1


def feistel(x, hb, s):
    """8 rounds on the 2*hb-bit value x, keyed by the 32-bit seed s."""
    hbs = np.uint64(hb)
    mh = np.uint64((1 << hb) - 1)
    x = _u(x)
    L, R = x >> hbs, x & mh
    for r in range(8):
        f = mix32(R ^ np.uint64((int(s) + r * GOLD) & 0xFFFFFFFF)) & mh
        L, R = R, L ^ f
    return (L << hbs) | R


def permute(i, m, s, walk=None):
    """The seeded bijection of [0, m) at i (scalar or array): feistel applied until the value is
    below m. `walk`, a one-element list, receives the largest number of applications."""
    i = np.atleast_1d(np.asarray(i, dtype=np.uint64)).copy()
    if m <= 1:
        return np.zeros(i.shape, np.int64)
    hb = half_bits(m)
    live = np.ones(i.shape, bool)
    steps = 0
    while live.any():
        i[live] = feistel(i[live], hb, s)
        live &= i >= np.uint64(m)
        steps += 1
    if walk is not None:
        walk[0] = max(walk[0], steps)
    return i.astype(np.int64)


def nais_seeds(seed):
    """(s0, s1) of nais_make_train_batch: the history order's seed and the negatives'."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lo, hi = seed & 0xFFFFFFFF, seed >> 32
    s0 = int(mix32(lo ^ 0x85EBCA6B))
    s1 = int(mix32(hi ^ ((lo * GOLD) & 0xFFFFFFFF)))
    return s0, s1


def bpr_user_seed(seed, u):
    """su of bpr_make_batch_kernel: nais_make_train_batch's s1, then one seed per user."""
    s1 = nais_seeds(seed)[1]
    return int(mix32(s1 ^ int(mix32((int(u) + GOLD) & 0xFFFFFFFF))))


def _first_free(row, P, count, draws, s):
    """The first `count` values of permute(k, P, s), k = 0 .. draws-1, that are not in `row`, in k
    order (fewer when the draws do not hold that many)."""
    cand = permute(np.arange(draws), P, s)
    return cand[~np.isin(cand, row)][:count]


def nais_batch(row, P, ng, seed):
    """make_batch_kernel for one sorted CSR row: (hist [n] int64, target [n (1 + ng)] int64,
    labels [n (1 + ng)] float32)."""
    row = np.asarray(row, np.int64)
    n = len(row)
    s0, s1 = nais_seeds(seed)
    hist = row[permute(np.arange(n), n, s0)] if n else row.copy()
    neg = _first_free(row, P, n * ng, n * (ng + 1), s1)
    assert len(neg) == n * ng, "n (1 + ng) <= P guarantees enough non-positives"
    target = np.concatenate([hist[:, None], neg.reshape(n, ng)], 1).reshape(-1)
    labels = np.tile(np.array([1.0] + [0.0] * ng, np.float32), n)
    return hist, target, labels


def bpr_batch(row, u, P, seed):
    """bpr_make_batch_kernel for one listed user: (user [h], item_i [h], item_j [h]) int64."""
    row = np.asarray(row, np.int64)
    h = len(row)
    neg = _first_free(row, P, h, 2 * h, bpr_user_seed(seed, u))
    assert len(neg) == h, "h <= P - h guarantees enough non-positives"
    return np.full(h, int(u), np.int64), row.copy(), neg
