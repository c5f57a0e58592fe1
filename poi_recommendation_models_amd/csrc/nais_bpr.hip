// nais_bpr.hip -- the BPR model (model.py:587-620) on gfx950: the batch forward and the fused
// full-catalog scorer + top-k (the user loop of validation.py:138-147). See include/nais.h "BPR".
//
// Scorer layout. A workgroup (4 waves) owns BPR_UT = 32 users and one column chunk. The 32 user
// rows sit in LDS for the whole chunk ([32][DP2 + 1], DP2 = D rounded up to even, the odd column
// zero). Per step every wave takes its own 32 candidates: their item rows are staged in LDS in K
// slices of BPR_KC floats ([32][BPR_KC + 1]; both pitches are odd, so lanes over rows read
// distinct banks), the next slice is fetched into registers while the current one runs
//   C (32 users x 32 candidates) += U_tile . I_tile^T        v_mfma_f32_32x32x2_f32, e ascending
// which is the fmaf chain over e = 0, 1, ..., DP2 - 1 of the forward kernel, bit for bit.
//
// No score is written. User u keeps tau_u, the key of its current k-th best (the key of -inf
// until it has k) and that key's score as a float. The epilogue does one float compare per score,
// !(score < tau's score), which NaN and -0 pass; a survivor's canonical ordered bits and POI id
// are then compared with tau_u as a whole key, and the key is appended to the user's
// LDS buffer (ds_add on its counter); the buffer's keys are looked up in the user's sorted CSR row
// when it is compacted, 64 lanes at a time, and history POIs dropped there. A step adds at
// most 32 * 4 = 128 keys per user, so a buffer of BPR_BUF = 256 that is compacted whenever it
// holds more than 128 after a step never overflows. Compaction (user slot s by wave s % 4, so a
// user's list has one reader and one writer): list (<= k, in the chunk's slice of the workspace)
// + buffer -> bitonic sort of <= 512 keys in LDS -> best k back to the list, tau_u = the k-th.
// With more than one column chunk the chunks of a user publish their tau in global memory
// (atomicMax) and take the highest, and a merge kernel keeps the best k of the chunks' lists; keys
// are unique and a published tau is always the k-th of k real candidates, so the result does not
// depend on the chunking or on which chunk runs first.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "nais_bpr_common.h"
#include "nais_internal.h"
#include "nais_topk_dev.h"

typedef float floatx16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int BPR_UT = 32;                  // users per workgroup (one MFMA tile)
constexpr int BPR_KC = 64;                  // K extent of one staged item slice
constexpr int BPR_IP = BPR_KC + 1;          // its LDS pitch
constexpr int64_t BPR_MIN_CHUNK = 2048;     // columns per chunk at least (the warm-up of tau)

__device__ __forceinline__ int crow(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

struct BP {
  int D;
  int64_t P;
  const float* U;
  const float* I;
};

// the dot product of the scorer: the fmaf chain over e ascending
__device__ __forceinline__ float bpr_dot(const float* __restrict__ a, const float* __restrict__ b,
                                         int D) {
  float s = 0.f;
  for (int e = 0; e < D; ++e) s = fmaf(a[e], b[e], s);
  return bpr_canon(s);
}

__global__ __launch_bounds__(256) void bpr_forward_kernel(
    BP p, int64_t num_users, const int64_t* __restrict__ user, const int64_t* __restrict__ item_i,
    const int64_t* __restrict__ item_j, int64_t n, float* __restrict__ out_i,
    float* __restrict__ out_j) {
  const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (t >= n) return;
  const float nan = __builtin_nanf("");
  const int64_t u = user[t], i = item_i[t];
  const bool uok = u >= 0 && u < num_users;
  out_i[t] = (uok && i >= 0 && i < p.P) ? bpr_dot(p.U + u * p.D, p.I + i * p.D, p.D) : nan;
  if (item_j) {
    const int64_t j = item_j[t];
    out_j[t] = (uok && j >= 0 && j < p.P) ? bpr_dot(p.U + u * p.D, p.I + j * p.D, p.D) : nan;
  }
}

__global__ __launch_bounds__(64 * BPR_NW) void bpr_score_topk_kernel(
    BP p, const int64_t* __restrict__ indptr, const int64_t* __restrict__ indices,
    const int32_t* __restrict__ users, int nu, int nut, int k, int64_t cpc,
    u64* __restrict__ keys, int32_t* __restrict__ kcount, u64* __restrict__ tau_g, int pu,
    int DP2) {
  extern __shared__ u64 bpr_lds[];
  u64* Lbuf = bpr_lds;                                   // [32][BPR_BUF]
  u64* Lsort = Lbuf + BPR_UT * BPR_BUF;                  // [BPR_NW][BPR_SORT]
  u64* Ltau = Lsort + BPR_NW * BPR_SORT;                 // [32]
  int64_t* Lbeg = reinterpret_cast<int64_t*>(Ltau + BPR_UT);   // [32] CSR row start
  int64_t* Luid = Lbeg + BPR_UT;                         // [32]
  int* Lh = reinterpret_cast<int*>(Luid + BPR_UT);       // [32] history length, -1: no such user
  int* Lcnt = Lh + BPR_UT;                               // [32] keys in the buffer
  int* Lln = Lcnt + BPR_UT;                              // [32] keys in the list
  int* Lneed = Lln + BPR_UT;                             // [4] (3 used) "a buffer wants compacting"
  float* Ltf = reinterpret_cast<float*>(Lneed + 4);      // [32] the score in tau, as a float
  float* Lu = Ltf + BPR_UT;                              // [32][pu]
  float* Lt = Lu + BPR_UT * pu;                          // [BPR_NW][32][BPR_IP]

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 31, hh = lane >> 5;
  const int D = p.D;
  const int ut = int(blockIdx.x % unsigned(nut)), ch = int(blockIdx.x / unsigned(nut));
  const int64_t c_begin = int64_t(ch) * cpc;
  const int64_t c_end = (c_begin + cpc < p.P) ? c_begin + cpc : p.P;
  const int slot0 = ut * BPR_UT;
  const float* __restrict__ Ip = p.I;

  if (tid < BPR_UT) {
    const int slot = slot0 + tid;
    int64_t u = 0, beg = 0;
    int h = -1;
    if (slot < nu) {
      u = users[slot];
      beg = indptr[u];
      h = int(indptr[u + 1] - beg);
    }
    Luid[tid] = u;
    Lbeg[tid] = beg;
    Lh[tid] = h;
    Lcnt[tid] = 0;
    Lln[tid] = 0;
    // no such user: a tau no key beats, so the slot never gets a survivor
    u64 t0 = (h >= 0) ? u64(ORD_NEG_INF) << 32 : ~0ull;
    if (tau_g && h >= 0) {   // what the user's other chunks have established so far
      const u64 g = __hip_atomic_load(tau_g + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (g > t0) t0 = g;
    }
    Ltau[tid] = t0;
    Ltf[tid] = (h >= 0) ? ord_score(uint32_t(t0 >> 32)) : INFINITY;
    if (tid < 4) Lneed[tid] = 0;
  }
  __syncthreads();
  for (int idx = tid; idx < BPR_UT * DP2; idx += 64 * BPR_NW) {
    const int r = idx / DP2, e = idx - r * DP2;
    Lu[r * pu + e] = (Lh[r] >= 0 && e < D) ? p.U[Luid[r] * D + e] : 0.f;
  }
  __syncthreads();

  float* Ltw = Lt + wave * 32 * BPR_IP;
  u64* S = Lsort + wave * BPR_SORT;
  const int nkc = (DP2 + BPR_KC - 1) / BPR_KC;
  const int64_t ntiles = (c_end - c_begin + BPR_STEP - 1) / BPR_STEP;

  // item rows [cb, cb + 32) x dims [k0, k0 + 64): lane = dim, register i = row; zero past the
  // chunk's last column and past D
  float pf[32];
  // Workgroups start their sweep at different steps (a rotation by user tile): they would
  // otherwise all ask the L2 for the same item rows at the same moment. A top-k does not depend
  // on the order its candidates are seen in.
  const int64_t rot = ntiles ? (int64_t(ut) * 37) % ntiles : 0;
  auto first_col = [&](int64_t tile) {
    int64_t t = tile + rot;
    if (t >= ntiles) t -= ntiles;
    return c_begin + t * BPR_STEP + 32 * wave;
  };
  // Every load is unconditional, from an address clamped into the table (the last dim, the
  // chunk's last row). The loaded registers are not touched here -- a select on them would make
  // the wave wait for the loads before the MFMAs they are meant to run under; the values that
  // do not count are dropped where the slice is written to LDS.
  int64_t pf_cb = 0;
  bool pf_eok = false;
  auto fetch = [&](int64_t tile, int kc) {
    const int64_t cb = first_col(tile);
    const int e = kc * BPR_KC + lane;
    pf_cb = cb;
    pf_eok = e < D;
    const float* __restrict__ q = Ip + (pf_eok ? e : D - 1);
    if (cb + 32 <= c_end) {
      q += cb * D;
#pragma unroll
      for (int i = 0; i < 32; ++i) pf[i] = q[int64_t(i) * D];
    } else {
#pragma unroll
      for (int i = 0; i < 32; ++i) pf[i] = q[((cb + i < c_end) ? cb + i : c_end - 1) * D];
    }
  };
  if (ntiles > 0) fetch(0, 0);

  for (int64_t tile = 0; tile < ntiles; ++tile) {
    floatx16 C;
#pragma unroll
    for (int r = 0; r < 16; ++r) C[r] = 0.f;
    for (int kc = 0; kc < nkc; ++kc) {
      wave_sync();   // this wave is done reading the previous slice
#pragma unroll
      for (int i = 0; i < 32; ++i)
        Ltw[i * BPR_IP + lane] = (pf_eok && pf_cb + i < c_end) ? pf[i] : 0.f;
      wave_sync();
      if (kc + 1 < nkc) fetch(tile, kc + 1);
      else if (tile + 1 < ntiles) fetch(tile + 1, 0);
      const int k0 = kc * BPR_KC;
      const int cw = (DP2 - k0 < BPR_KC) ? DP2 - k0 : BPR_KC;
      const float* ap = Lu + n * pu + k0 + hh;
      const float* bp = Ltw + n * BPR_IP + hh;
#pragma unroll 8
      for (int kk = 0; kk < cw; kk += 2)
        C = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk], bp[kk], C, 0, 0, 0);
    }

    // epilogue: lane (n, hh) holds candidate c for the 16 users crow(r, hh). Their thresholds are
    // read first, all at once (they change only in a compaction, behind a barrier).
    const int64_t c = first_col(tile) + n;
    const bool valid = c < c_end;
    const uint32_t idw = 0xFFFFFFFFu - uint32_t(c);
    const int ph = int(tile % 3);
    float tf[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) tf[r] = Ltf[crow(r, hh)];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      // one compare per score: below tau's score (as floats; a NaN on either side passes) it is
      // no survivor. The rest is the rare path: the ordered bits and the whole key against tau.
      if (valid && !(C[r] < tf[r])) {
        const int ur = crow(r, hh);
        const u64 tau = Ltau[ur];
        const u64 key = (u64(ord_bits(bpr_canon(C[r]))) << 32) | u64(idw);
        if (key > tau) {
          const int pos = atomicAdd(&Lcnt[ur], 1);
          if (pos < BPR_BUF) Lbuf[ur * BPR_BUF + pos] = key;   // always true (see the bounds)
          if (pos >= BPR_TRIG) Lneed[ph] = 1;
        }
      }
    }
    __syncthreads();

    // Most steps compact nothing and have this one barrier. The flag of step t + 2 is cleared
    // here: it was last read in step t - 1, and is next set after the barrier of step t + 1.
    const bool last = tile + 1 == ntiles;
    const bool need = Lneed[ph] != 0 || last;
    if (tid == 0) Lneed[(ph + 2) % 3] = 0;
    if (!need) continue;
    for (int ur = wave; ur < BPR_UT; ur += BPR_NW) {
      const int cnt = Lcnt[ur];   // wave-uniform
      if (cnt > BPR_TRIG || (last && cnt > 0)) {
        const int ln = Lln[ur];
        int tot = ln + cnt;
        u64* list = keys + (int64_t(ch) * nu + slot0 + ur) * k;
        const int n2 = pow2_at_least(tot);
        // the buffer's keys are looked up in the history here, 64 at a time (one dependent chain
        // of loads per 64 survivors instead of one per survivor); a history POI becomes key 0
        const int h = Lh[ur];
        const int64_t* __restrict__ hist = indices + Lbeg[ur];
        int removed = 0;
        for (int i = lane; i < n2; i += 64) {
          u64 v = 0ull;
          if (i < ln) v = list[i];
          else if (i < tot) {
            v = Lbuf[ur * BPR_BUF + (i - ln)];
            const int64_t cv = int64_t(0xFFFFFFFFu - uint32_t(v));
            int lo = 0, hi = h;
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (hist[mid] < cv) lo = mid + 1; else hi = mid;
            }
            if (lo < h && hist[lo] == cv) v = 0ull;
          }
          removed += __popcll(__ballot(i >= ln && i < tot && v == 0ull));
          S[i] = v;
        }
        tot -= removed;
        wave_sort_desc(S, n2, lane);
        const int nl = (tot < k) ? tot : k;
        for (int i = lane; i < nl; i += 64) list[i] = S[i];
        if (lane == 0) {
          Lln[ur] = nl;
          Lcnt[ur] = 0;
          // tau: the k-th key of this chunk's list, or what another chunk of the same user has
          // published if that is higher. Either is the k-th best of k candidates the user
          // really has, so no key below it can be among the user's best k.
          u64 t = (nl == k) ? S[k - 1] : 0ull;
          if (tau_g) {
            u64* gp = tau_g + slot0 + ur;
            const u64 g = (nl == k) ? atomicMax(gp, t)
                                    : __hip_atomic_load(gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (g > t) t = g;
          }
          if (t > Ltau[ur]) {
            Ltau[ur] = t;
            Ltf[ur] = ord_score(uint32_t(t >> 32));
          }
        }
        wave_sync();
      }
    }
    __syncthreads();
  }
  if (tid < BPR_UT && slot0 + tid < nu) kcount[int64_t(ch) * nu + slot0 + tid] = Lln[tid];
}

// Column chunks of a job (topk_chunking): a workgroup is one tile of BPR_UT users.
void chunking(int64_t P, int nu, int k, int want, int* nchunks, int64_t* cpc) {
  topk_chunking(P, (nu + BPR_UT - 1) / BPR_UT, k, want, BPR_MIN_CHUNK, nchunks, cpc);
}

}  // namespace

extern "C" {

int32_t nais_bpr_forward(const nais_bpr_params_t* params, const int64_t* user,
                         const int64_t* item_i, const int64_t* item_j, int64_t n, float* out_i,
                         float* out_j, void* stream) {
  if (int rc = nais_bpr_check_params(params)) return rc;
  if (n < 0) return nais_internal_fail(NAIS_E_INVALID, "bad shape");
  if (n == 0) return NAIS_OK;
  if (n > (int64_t(0x7fffffff) << 8)) return nais_internal_fail(NAIS_E_UNSUPPORTED, "n too large");
  if (!user || !item_i || !out_i || ((item_j != nullptr) != (out_j != nullptr)))
    return nais_internal_fail(NAIS_E_INVALID, "NULL pointer (item_j and out_j go together)");
  BP p{params->embed_dim, params->num_pois, params->embed_user, params->embed_item};
  hipLaunchKernelGGL(bpr_forward_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), p, params->num_users, user, item_i,
                     item_j, n, out_i, out_j);
  return nais_internal_check_launch("bpr_forward_kernel");
}

size_t nais_bpr_score_topk_workspace_size(const nais_bpr_params_t* params, int32_t num_users,
                                          int32_t k, int32_t num_chunks) {
  if (!params || num_users <= 0 || k <= 0 || params->num_pois < 1) return 0;
  int nc;
  int64_t cpc;
  chunking(params->num_pois, num_users, k, num_chunks, &nc, &cpc);
  return topk_ws_bytes(num_users, k, nc);
}

int32_t nais_bpr_score_topk(const nais_bpr_params_t* params, const int64_t* indptr,
                            const int64_t* indices, const int32_t* users, int32_t num_users,
                            int32_t k, int32_t num_chunks, uint64_t* keys, int32_t* kcount,
                            void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = nais_bpr_check_params(params)) return rc;
  if (num_users < 0 || num_chunks < 0) return nais_internal_fail(NAIS_E_INVALID, "bad shape");
  if (k < 1 || k > 256) return nais_internal_fail(NAIS_E_UNSUPPORTED, "k must be 1..256");
  if (num_users == 0) return NAIS_OK;
  if (!indptr || !users || !keys || !kcount)   // indices may be NULL: a CSR without entries
    return nais_internal_fail(NAIS_E_INVALID, "NULL pointer");
  int nc;
  int64_t cpc;
  chunking(params->num_pois, num_users, k, num_chunks, &nc, &cpc);
  const size_t need = topk_ws_bytes(num_users, k, nc);
  if (need && (!workspace || workspace_bytes < need))
    return nais_internal_fail(NAIS_E_WORKSPACE, "workspace missing or too small");
  const int nut = (num_users + BPR_UT - 1) / BPR_UT;
  if (int64_t(nut) * nc > 0x7fffffffll) return nais_internal_fail(NAIS_E_UNSUPPORTED, "job too large");
  const int D = params->embed_dim, DP2 = (D + 1) & ~1, pu = DP2 + 1;
  const size_t lds = size_t(BPR_UT * BPR_BUF + BPR_NW * BPR_SORT + 3 * BPR_UT) * 8 +
                     size_t(4 * BPR_UT + 4) * 4 + size_t(BPR_UT * pu + BPR_NW * 32 * BPR_IP) * 4;
  static bool once = (hipFuncSetAttribute(reinterpret_cast<const void*>(bpr_score_topk_kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024),
                      true);
  (void)once;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  u64* wk = (nc > 1) ? static_cast<u64*>(workspace) : reinterpret_cast<u64*>(keys);
  u64* tg = (nc > 1) ? wk + size_t(nc) * num_users * k : nullptr;
  int32_t* wc = (nc > 1) ? reinterpret_cast<int32_t*>(tg + num_users) : kcount;
  if (tg && hipMemsetAsync(tg, 0, size_t(num_users) * sizeof(u64), st) != hipSuccess)
    return nais_internal_fail(NAIS_E_HIP, "hipMemsetAsync failed");
  BP p{D, params->num_pois, params->embed_user, params->embed_item};
  hipLaunchKernelGGL(bpr_score_topk_kernel, dim3((unsigned)(nut * nc)), dim3(64 * BPR_NW), lds, st,
                     p, indptr, indices, users, (int)num_users, nut, (int)k, cpc, wk, wc, tg, pu, DP2);
  if (int rc = nais_internal_check_launch("bpr_score_topk_kernel")) return rc;
  if (nc > 1) {
    hipLaunchKernelGGL(bpr_merge_kernel, dim3((unsigned)num_users), dim3(64), 0, st, wk, wc,
                       (int)num_users, nc, (int)k, reinterpret_cast<u64*>(keys), kcount);
    return nais_internal_check_launch("bpr_merge_kernel");
  }
  return NAIS_OK;
}

}  // extern "C"
