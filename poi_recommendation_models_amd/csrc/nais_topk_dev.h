// nais_topk_dev.h -- device helpers of the fused scorer + top-k kernels (nais_bpr.hip,
// nais_new1.hip; not ABI): the key format of nais_topk_keys_finish, the survivor-buffer geometry,
// the wave-level bitonic sort and the kernel that merges the column chunks' lists. Everything
// sits in the including translation unit's anonymous namespace.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "nais_internal.h"

namespace {

constexpr int BPR_NW = 4;                   // waves per workgroup, 32 candidates each per step
constexpr int BPR_STEP = 32 * BPR_NW;       // candidates per workgroup step
constexpr int BPR_BUF = 256;                // survivor keys per user
constexpr int BPR_TRIG = BPR_BUF - BPR_STEP;   // compact when a buffer holds more than this
constexpr int BPR_SORT = 512;               // k + BPR_BUF <= 512 keys per compaction
static_assert(BPR_TRIG + BPR_STEP <= BPR_BUF && 256 + BPR_BUF <= BPR_SORT, "buffer bounds");

typedef unsigned long long u64;
constexpr uint32_t ORD_NEG_INF = 0x007FFFFFu;   // ordered bits of -inf

__device__ __forceinline__ uint32_t ord_bits(float f) {   // f canonical (bpr_canon)
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the score whose ordered bits are o
__device__ __forceinline__ float ord_score(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// descending bitonic sort of S[0..n2), n2 a power of two in [64, BPR_SORT], by one wave. A stage
// reads its (up to four) pairs per lane first and then writes them all, so it costs two LDS
// round trips, not one per pair.
__device__ __forceinline__ void wave_sort_desc(u64* S, int n2, int lane) {
  const int half = n2 >> 1;
  for (int size = 2; size <= n2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      wave_sync();
      u64 a[BPR_SORT / 128], b[BPR_SORT / 128];
#pragma unroll
      for (int x = 0; x < BPR_SORT / 128; ++x) {
        const int t = lane + 64 * x;
        const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));
        if (t < half) {
          a[x] = S[i];
          b[x] = S[i + stride];
        }
      }
#pragma unroll
      for (int x = 0; x < BPR_SORT / 128; ++x) {
        const int t = lane + 64 * x;
        const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));
        if (t < half) {
          const bool desc = (i & size) == 0;
          const u64 hi = (a[x] > b[x]) ? a[x] : b[x], lo = (a[x] > b[x]) ? b[x] : a[x];
          S[i] = desc ? hi : lo;
          S[i + stride] = desc ? lo : hi;
        }
      }
    }
  }
  wave_sync();
}

__device__ __forceinline__ int pow2_at_least(int n) {
  int p = 64;
  while (p < n) p <<= 1;
  return p;
}

// A score as the kernels report it: the value with -0 folded into +0 (x + 0; for an odd BPR
// width that is also the zero pair the MFMA adds) and every NaN the one quiet NaN a key can carry.
__device__ __forceinline__ float bpr_canon(float s) {
  s += 0.f;
  return (s != s) ? __uint_as_float(0x7FC00000u) : s;
}

// best k of the chunks' lists: one wave per user
__global__ __launch_bounds__(64) void bpr_merge_kernel(const u64* __restrict__ ws_keys,
                                                       const int32_t* __restrict__ ws_cnt, int nu,
                                                       int nchunks, int k, u64* __restrict__ keys,
                                                       int32_t* __restrict__ kcount) {
  __shared__ u64 S[BPR_SORT];
  const int slot = blockIdx.x, lane = threadIdx.x;
  int ln = 0;
  for (int ch = 0; ch < nchunks; ++ch) {
    int cnt = ws_cnt[int64_t(ch) * nu + slot];
    cnt = (cnt < 0) ? 0 : ((cnt > k) ? k : cnt);
    const u64* src = ws_keys + (int64_t(ch) * nu + slot) * k;
    const int tot = ln + cnt, n2 = pow2_at_least(tot);
    wave_sync();
    for (int i = ln + lane; i < n2; i += 64) S[i] = (i < tot) ? src[i - ln] : 0ull;
    wave_sort_desc(S, n2, lane);
    ln = (tot < k) ? tot : k;
  }
  for (int i = lane; i < ln; i += 64) keys[int64_t(slot) * k + i] = S[i];
  if (lane == 0) kcount[slot] = ln;
}

// workspace of a chunked job: the chunks' lists, the users' shared tau, the chunks' counts
inline size_t topk_ws_bytes(int nu, int k, int nchunks) {
  if (nchunks <= 1) return 0;
  return size_t(nchunks) * nu * (size_t(k) * sizeof(u64) + sizeof(int32_t)) +
         size_t(nu) * sizeof(u64) + 16;
}

// Column chunks of a job of `nwg` workgroups per chunk, each sweeping `steps` candidate steps. One
// workgroup fits a CU, so a job runs in ceil(nwg * nc / CUs) rounds of 1 / nc of a workgroup's
// sweep each: nc is the count (up to 32, no chunk below min_chunk columns or 16 k) with the least
// rounds / nc, each chunk charged 2 % for its own start. The chunks of a user share tau, so a
// later chunk does not warm up from -inf.
inline void topk_chunking(int64_t P, int64_t nwg, int k, int want, int64_t min_chunk, int* nchunks,
                          int64_t* cpc) {
  const int64_t steps = (P + BPR_STEP - 1) / BPR_STEP;
  int64_t nc = want;
  if (nc <= 0) {
    int cus = nais_internal_stream_cus(nullptr);
    if (cus <= 0) cus = 256;
    const int64_t min_cols = std::max<int64_t>(min_chunk, 16 * int64_t(k));
    const int64_t most = std::max<int64_t>(1, std::min<int64_t>(32, P / min_cols));
    double best = 0.0;
    for (int64_t c = 1; c <= most; ++c) {
      const double cost = double((nwg * c + cus - 1) / cus) / double(c) * (1.0 + 0.02 * double(c));
      if (c == 1 || cost < best) {
        best = cost;
        nc = c;
      }
    }
  }
  nc = std::max<int64_t>(1, std::min<int64_t>(nc, steps));
  const int64_t per = (steps + nc - 1) / nc;
  *cpc = per * BPR_STEP;
  *nchunks = int((steps + per - 1) / per);
}

}  // namespace
