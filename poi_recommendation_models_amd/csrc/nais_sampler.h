// nais_sampler.h -- the seeded permutation behind the device-side batch builders
// (nais_make_train_batch, nais_bpr_make_train_batch): a uniformly random distinct subset of
// [0, m) is the first members of a pseudo-random order of [0, m), which comes from a seeded
// Feistel permutation of [0, 4^h) walked down to [0, m) (cycle walking), so no sort is needed.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

__host__ __device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// 8-round Feistel network on [0, 2^(2*hb)) keyed by the seed (round function: murmur finaliser;
// 8 rounds: 4 leave a visible bias on domains of a few elements)
__device__ __forceinline__ uint32_t feistel(uint32_t x, int hb, uint32_t s) {
  const uint32_t mh = (1u << hb) - 1u;
  uint32_t L = x >> hb, R = x & mh;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint32_t f = mix32(R ^ (s + uint32_t(r) * 0x9e3779b9u)) & mh;
    const uint32_t t = L ^ f;
    L = R;
    R = t;
  }
  return (L << hb) | R;
}

// bijection of [0, m): the Feistel permutation of [0, 2^(2 hb)) >= m, walked until it lands < m
__device__ __forceinline__ uint32_t permute(uint32_t i, uint32_t m, int hb, uint32_t s) {
  do {
    i = feistel(i, hb, s);
  } while (i >= m);
  return i;
}

// half the bits of the smallest power of two >= m (m >= 2), rounded up
__device__ __forceinline__ int half_bits(uint32_t m) {
  const int k = 32 - __clz(m - 1);
  return (k + 1) >> 1;
}
