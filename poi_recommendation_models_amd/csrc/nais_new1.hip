// nais_new1.hip -- the New1 model (model.py:830-925) on gfx950: the batch forward, the catalog
// tables T / Q / K / V and the fused per-user scorer + top-k (the user loop of
// validation.py:212-230). See include/nais.h "New1" and DESIGN.md "New1".
//
// With t_c the candidate's concatenated row, h_j a history item's, q_c = Wq t_c, K_j = Wk h_j,
// V_j = Wv h_j, and Kflat the row's contiguous [n, d] key buffer (Kflat[j * d + k] = K_j[k]):
//   a_j'  = sum_e q_c[e] * Kflat[e * n + j'] / sqrtf(d)      (model.py:896: a reshape, no transpose)
//   e_j   = expf(a_j) * [hist_j != c]                        (no max-subtraction)
//   pred  = sum_j (e_j / powf(sum_j e_j, beta)) * (V_j . t_c)  +  t_c . sum_j r_j h_j
// In evaluation every row of a user shares the history, so Q, K, V are per-POI tables (one GEMM
// over the catalog) and a user costs two [C, d] x [d, n] products and a streaming epilogue.
//
// Scorer layout. A workgroup (4 waves) owns one user and one column chunk. LDS holds a block of
// the history: Lk[e][j'] = Kflat[e * n + jb0 + j'] (pitch = the block's rows rounded up to 32:
// lanes over j' read consecutive banks) and Lv[j][k] = V[hist_j][k] (pitch d + 1, odd), plus
// g = sum_j r_j h_j. Per step every wave takes its own 32 candidates: lane (c, hh) keeps q_c[k]
// and t_c[k] for k = hh (mod 2) in registers (d <= 128; read from the tables in the loop above
// that) and walks the block's 32-row tiles with two v_mfma_f32_32x32x2_f32 chains over k,
//   C1 (32 j x 32 c) = Lk^T . Q^T        C2 (32 j x 32 c) = Lv . T^T
// then adds expf(C1 / sqrtf(d)) and expf(..) * C2 over its 16 rows into two running sums; the two
// lane halves are added at the end. A history longer than the block (JB rows, from the LDS budget)
// is walked block by block over supersteps of N1_SUPER steps, the lanes' running sums parked in
// LDS between blocks: the sums need no rescaling. No score is written: the survivor buffer, tau
// and the compaction are those of nais_bpr.hip (nais_topk_dev.h), for one user per workgroup.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "nais_internal.h"
#include "nais_topk_dev.h"

typedef float floatx16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int N1_SUPER = 8;                 // steps per superstep of the j-tiled route
constexpr int N1_MAXJB = 2048;              // rows of a history block at most
constexpr int64_t N1_MIN_CHUNK = 2048;      // columns per chunk at least (the warm-up of tau)
// LDS before the history block: buffer, sort space, tau (padded), 7 ints (padded), g, parked sums
constexpr size_t N1_FIXED = size_t(BPR_BUF + BPR_SORT + 2) * 8 + 32 + 256 * 4 +
                            size_t(N1_SUPER) * 64 * BPR_NW * 2 * 4;
constexpr size_t N1_LDS = 160 * 1024;

__device__ __forceinline__ int crow(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

struct NP1 {
  int d;
  int64_t P, R;
  float beta;
  const float *E, *Er, *Wq, *Wk, *Wv;
};

int check_params(const nais_new1_params_t* q) {
  if (!q) return nais_internal_fail(NAIS_E_INVALID, "NULL params");
  if (q->embed_dim < 2 || q->embed_dim > 256 || (q->embed_dim & 1))
    return nais_internal_fail(NAIS_E_UNSUPPORTED, "New1 embed_dim must be even, 2..256");
  if (q->hidden != q->embed_dim)
    return nais_internal_fail(NAIS_E_UNSUPPORTED,
                              "New1 hidden must equal embed_dim (the reshape of model.py:896)");
  if (q->num_pois < 1 || q->num_regions < 1) return nais_internal_fail(NAIS_E_INVALID, "bad shape");
  if (q->num_pois >= (int64_t(1) << 24))
    return nais_internal_fail(NAIS_E_UNSUPPORTED, "New1 num_pois must be below 2^24");
  if (!q->embed_target || !q->embed_region || !q->attn_q || !q->attn_k || !q->attn_v)
    return nais_internal_fail(NAIS_E_INVALID, "NULL parameter pointer");
  return NAIS_OK;
}

NP1 pack(const nais_new1_params_t* q) {
  return NP1{q->embed_dim, q->num_pois,  q->num_regions, q->beta,  q->embed_target,
             q->embed_region, q->attn_q, q->attn_k,      q->attn_v};
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// ---- forward: one wave per row; nothing of the row is stored, K and V elements are formed where
// they are used (the correctness path: d * d work per key element)
__global__ __launch_bounds__(256) void new1_forward_kernel(
    NP1 p, const int64_t* __restrict__ hist, int64_t hs, const int64_t* __restrict__ target,
    const int64_t* __restrict__ hreg, const int64_t* __restrict__ treg,
    const float* __restrict__ vr, int64_t b, int64_t n, float* __restrict__ out) {
  extern __shared__ float new1_fwd_lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int d = p.d, half = d >> 1;
  const int64_t row = int64_t(blockIdx.x) * 4 + wave;
  if (row >= b) return;   // whole waves leave; the rest of the kernel has no workgroup barrier
  float* Lt = new1_fwd_lds + wave * 2 * d;
  float* Lq = Lt + d;
  const int64_t* __restrict__ hrow = hist + row * hs;
  const int64_t* __restrict__ rrow = hreg + row * hs;
  const int64_t c = target[row], tr = treg[row];
  bool ok = c >= 0 && c < p.P && tr >= 0 && tr < p.R;
  for (int64_t j = lane; j < n; j += 64)
    ok = ok && hrow[j] >= 0 && hrow[j] < p.P && rrow[j] >= 0 && rrow[j] < p.R;
  if (!__all(ok)) {   // an id outside its table: the row reads nothing and is NaN
    if (lane == 0) out[row] = __builtin_nanf("");
    return;
  }
  for (int e = lane; e < d; e += 64)
    Lt[e] = (e < half) ? p.E[c * half + e] : p.Er[tr * half + (e - half)];
  wave_sync();
  for (int o = lane; o < d; o += 64) {
    float s = 0.f;
    for (int k = 0; k < d; ++k) s = fmaf(Lt[k], p.Wq[o * d + k], s);
    Lq[o] = s;
  }
  wave_sync();
  auto h = [&](int64_t j, int m) {
    return (m < half) ? p.E[hrow[j] * half + m] : p.Er[rrow[j] * half + (m - half)];
  };
  const float sqd = sqrtf(float(d));
  auto expa = [&](int64_t jp) {   // e_j' of the scrambled key buffer, masked as exp_A * mask
    float a = 0.f;
    for (int e = 0; e < d; ++e) {
      const int64_t x = int64_t(e) * n + jp, jj = x / d;
      const int kk = int(x - jj * d);
      float s = 0.f;
      for (int m = 0; m < d; ++m) s = fmaf(h(jj, m), p.Wk[kk * d + m], s);
      a = fmaf(Lq[e], s, a);
    }
    return expf(a / sqd) * ((hrow[jp] != c) ? 1.f : 0.f);
  };
  float S = 0.f;
  for (int64_t j = lane; j < n; j += 64) S += expa(j);
  S = wave_sum(S);
  const float pw = powf(S, p.beta);
  float acc = 0.f;
  for (int64_t j = lane; j < n; j += 64) {
    const float w = expa(j) / pw, r = vr[j];
    for (int k = 0; k < d; ++k) {
      float v = 0.f;
      for (int m = 0; m < d; ++m) v = fmaf(h(j, m), p.Wv[k * d + m], v);
      acc = fmaf(fmaf(w, v, r * h(j, k)), Lt[k], acc);
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) out[row] = sigmoidf((n == 0) ? 0.f : acc);
}

// ---- catalog tables: 32 POIs per workgroup; T in LDS, the 3 * ceil(d / 32) output tiles over
// the waves, each one v_mfma_f32_32x32x2_f32 chain over k ascending (exact fp32)
__global__ __launch_bounds__(256) void new1_tables_kernel(
    NP1 p, const int64_t* __restrict__ region_of, float* __restrict__ T, float* __restrict__ Q,
    float* __restrict__ K, float* __restrict__ V) {
  extern __shared__ float new1_tab_lds[];   // [32][d + 1]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 31, hh = lane >> 5;
  const int d = p.d, half = d >> 1, pt = d + 1;
  const int64_t p0 = int64_t(blockIdx.x) * 32;
  for (int idx = tid; idx < 32 * d; idx += 256) {
    const int r = idx / d, e = idx - r * d;
    const int64_t poi = p0 + r;
    float v = 0.f;
    if (poi < p.P) {
      if (e < half) {
        v = p.E[poi * half + e];
      } else {   // a region outside the table: the POI's rows are NaN
        const int64_t rg = region_of[poi];
        v = (rg >= 0 && rg < p.R) ? p.Er[rg * half + (e - half)] : __builtin_nanf("");
      }
      T[poi * d + e] = v;
    }
    new1_tab_lds[r * pt + e] = v;
  }
  __syncthreads();
  const int nct = (d + 31) >> 5;
  for (int t = wave; t < 3 * nct; t += 4) {
    const int m = t / nct, ct = t - m * nct;
    const float* __restrict__ W = (m == 0) ? p.Wq : (m == 1) ? p.Wk : p.Wv;
    float* __restrict__ O = (m == 0) ? Q : (m == 1) ? K : V;
    const int o = ct * 32 + n, oc = (o < d) ? o : d - 1;
    const float* __restrict__ wp = W + int64_t(oc) * d + hh;
    const float* ap = new1_tab_lds + n * pt + hh;
    floatx16 C;
#pragma unroll
    for (int r = 0; r < 16; ++r) C[r] = 0.f;
#pragma unroll 4
    for (int kk = 0; kk < d; kk += 2)
      C = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk], wp[kk], C, 0, 0, 0);
    if (o < d) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t poi = p0 + crow(r, hh);
        if (poi < p.P) O[poi * d + o] = C[r];
      }
    }
  }
}

// ---- the scorer. NPR: k pairs a lane keeps of q_c and t_c (d <= 2 * NPR); 0: read in the loop.
template <int NPR>
__global__ __launch_bounds__(64 * BPR_NW) void new1_score_topk_kernel(
    int d, int64_t P, float beta, const float* __restrict__ T, const float* __restrict__ Q,
    const float* __restrict__ K, const float* __restrict__ V, const int64_t* __restrict__ indptr,
    const int64_t* __restrict__ indices, const float* __restrict__ vr,
    const int32_t* __restrict__ users, int nu, int k, int64_t cpc, u64* __restrict__ keys,
    int32_t* __restrict__ kcount, u64* __restrict__ tau_g, int JB) {
  extern __shared__ u64 new1_lds[];
  u64* Lbuf = new1_lds;                                  // [BPR_BUF]
  u64* Lsort = Lbuf + BPR_BUF;                           // [BPR_SORT]
  u64* Ltau = Lsort + BPR_SORT;                          // [1] (+ 1 pad)
  int* Lcnt = reinterpret_cast<int*>(Ltau + 2);          // keys in the buffer
  int* Lln = Lcnt + 1;                                   // keys in the list
  int* Lneed = Lln + 1;                                  // [4] (3 used) "the buffer wants compacting"
  float* Ltf = reinterpret_cast<float*>(Lneed + 4);      // the score in tau, as a float (+ 1 pad)
  float* Lg = Ltf + 2;                                   // [256] g = sum_j r_j h_j
  float* Lacc = Lg + 256;                                // [N1_SUPER][256][2] parked running sums
  float* Lk = Lacc + N1_SUPER * 64 * BPR_NW * 2;         // [d][pk]
  float* Lv = Lk + size_t(d) * JB;                       // [JB][d + 1]

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, cn = lane & 31, hh = lane >> 5;
  const int slot = int(blockIdx.x % unsigned(nu)), ch = int(blockIdx.x / unsigned(nu));
  const int64_t c_begin = int64_t(ch) * cpc;
  const int64_t c_end = (c_begin + cpc < P) ? c_begin + cpc : P;
  const int64_t u = users[slot], beg = indptr[u];
  const int n = int(indptr[u + 1] - beg);
  const int64_t* __restrict__ hist = indices + beg;
  const int pv = d + 1;
  const int n32 = (n + 31) & ~31;
  const int pk = (n32 < JB) ? ((n32 > 32) ? n32 : 32) : JB;
  const float sqd = sqrtf(float(d));

  if (tid == 0) {
    *Lcnt = 0;
    *Lln = 0;
    Lneed[0] = Lneed[1] = Lneed[2] = Lneed[3] = 0;
    u64 t0 = u64(ORD_NEG_INF) << 32;
    if (tau_g) {   // what the user's other chunks have established so far
      const u64 g = __hip_atomic_load(tau_g + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (g > t0) t0 = g;
    }
    *Ltau = t0;
    *Ltf = ord_score(uint32_t(t0 >> 32));
  }
  for (int e = tid; e < d; e += 64 * BPR_NW) {
    float s = 0.f;
    for (int j = 0; j < n; ++j) s = fmaf(vr[beg + j], T[hist[j] * d + e], s);
    Lg[e] = s;
  }

  const int nblk = (n > JB) ? (n + JB - 1) / JB : 1;
  const int64_t ntiles = (c_end - c_begin + BPR_STEP - 1) / BPR_STEP;
  const int64_t sps = (nblk > 1) ? N1_SUPER : ((ntiles > 0) ? ntiles : 1);
  u64* list = keys + (int64_t(ch) * nu + slot) * k;

  for (int64_t s0 = 0; s0 < ntiles; s0 += sps) {
    const int64_t s1 = (s0 + sps < ntiles) ? s0 + sps : ntiles;
    for (int blk = 0; blk < nblk; ++blk) {
      const int jb0 = blk * JB;
      const int jw = (n - jb0 < JB) ? n - jb0 : JB;      // rows of this block (0 for no history)
      const int jwp = (jw + 31) & ~31;                   // <= pk
      if (nblk > 1 || s0 == 0) {
        __syncthreads();   // every wave is done with the previous block
        for (int idx = tid; idx < d * jwp; idx += 64 * BPR_NW) {
          const int e = idx / jwp, jj = idx - e * jwp;
          float v = 0.f;
          if (jj < jw) {   // the [n, d] key buffer of the user re-read as [d, n]
            const int64_t x = int64_t(e) * n + jb0 + jj, hj = x / d;
            v = K[hist[hj] * d + (x - hj * d)];
          }
          Lk[e * pk + jj] = v;
        }
        for (int idx = tid; idx < jwp * d; idx += 64 * BPR_NW) {
          const int jj = idx / d, kk = idx - jj * d;
          Lv[jj * pv + kk] = (jj < jw) ? V[hist[jb0 + jj] * d + kk] : 0.f;
        }
        __syncthreads();
      }
      const bool last_blk = blk + 1 == nblk;
      for (int64_t step = s0; step < s1; ++step) {
        const int64_t c = c_begin + step * BPR_STEP + 32 * wave + cn;
        const int64_t cc = (c < c_end) ? c : c_end - 1;   // loads stay inside the tables
        const float* __restrict__ qrow = Q + cc * d + hh;
        const float* __restrict__ trow = T + cc * d + hh;
        float qreg[NPR ? NPR : 1], treg[NPR ? NPR : 1];
        if (NPR) {
#pragma unroll
          for (int i = 0; i < NPR; ++i) {
            const bool in = 2 * i < d;
            qreg[i] = in ? qrow[2 * i] : 0.f;
            treg[i] = in ? trow[2 * i] : 0.f;
          }
        }
        float S = 0.f, N = 0.f;
        float* park = Lacc + (size_t(step - s0) * 64 * BPR_NW + tid) * 2;
        if (blk > 0) {
          S = park[0];
          N = park[1];
        }
        for (int jt = 0; jt < jwp; jt += 32) {
          floatx16 C1, C2;
#pragma unroll
          for (int r = 0; r < 16; ++r) C1[r] = C2[r] = 0.f;
          const float* ka = Lk + hh * pk + jt + cn;
          const float* va = Lv + (jt + cn) * pv + hh;
          if (NPR) {
#pragma unroll
            for (int i = 0; i < NPR; ++i) {
              if (2 * i < d) {
                C1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[2 * i * pk], qreg[i], C1, 0, 0, 0);
                C2 = __builtin_amdgcn_mfma_f32_32x32x2f32(va[2 * i], treg[i], C2, 0, 0, 0);
              }
            }
          } else {
            for (int kk = 0; kk < d; kk += 2) {
              C1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[kk * pk], qrow[kk], C1, 0, 0, 0);
              C2 = __builtin_amdgcn_mfma_f32_32x32x2f32(va[kk], trow[kk], C2, 0, 0, 0);
            }
          }
          // lane (c, hh) holds candidate c for the 16 history rows jt + crow(r, hh)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float e = (jt + crow(r, hh) < jw) ? expf(C1[r] / sqd) : 0.f;
            S += e;
            N = fmaf(e, C2[r], N);
          }
        }
        if (!last_blk) {   // workgroup-uniform
          park[0] = S;
          park[1] = N;
          continue;
        }
        float gd = 0.f;
        if (NPR) {
#pragma unroll
          for (int i = 0; i < NPR; ++i)
            if (2 * i < d) gd = fmaf(treg[i], Lg[2 * i + hh], gd);
        } else {
          for (int kk = 0; kk < d; kk += 2) gd = fmaf(trow[kk], Lg[kk + hh], gd);
        }
        S += __shfl_xor(S, 32);
        N += __shfl_xor(N, 32);
        gd += __shfl_xor(gd, 32);
        const float pred = (n == 0) ? 0.f : N / powf(S, beta) + gd;
        const float score = bpr_canon(sigmoidf(pred));
        const int ph = int(step % 3);
        // one compare per score: below tau's score (a NaN on either side passes) it is no
        // survivor; else the whole key against tau
        if (hh == 0 && c < c_end && !(score < *Ltf)) {
          const u64 key = (u64(ord_bits(score)) << 32) | u64(0xFFFFFFFFu - uint32_t(c));
          if (key > *Ltau) {
            const int pos = atomicAdd(Lcnt, 1);
            if (pos < BPR_BUF) Lbuf[pos] = key;   // always true: <= BPR_STEP keys per step
            if (pos >= BPR_TRIG) Lneed[ph] = 1;
          }
        }
        __syncthreads();

        // Most steps compact nothing and have this one barrier. The flag of step t + 2 is cleared
        // here: it was last read in step t - 1, and is next set after the barrier of step t + 1.
        const bool last = step + 1 == ntiles;
        const bool need = Lneed[ph] != 0 || last;
        if (tid == 0) Lneed[(ph + 2) % 3] = 0;
        if (!need) continue;
        if (wave == 0) {
          const int cnt = *Lcnt;
          if (cnt > BPR_TRIG || (last && cnt > 0)) {
            const int ln = *Lln;
            int tot = ln + cnt;
            const int n2 = pow2_at_least(tot);
            // the buffer's keys are looked up in the sorted history here; a history POI becomes 0
            int removed = 0;
            for (int i = lane; i < n2; i += 64) {
              u64 v = 0ull;
              if (i < ln) v = list[i];
              else if (i < tot) {
                v = Lbuf[i - ln];
                const int64_t cv = int64_t(0xFFFFFFFFu - uint32_t(v));
                int lo = 0, hi = n;
                while (lo < hi) {
                  const int mid = (lo + hi) >> 1;
                  if (hist[mid] < cv) lo = mid + 1; else hi = mid;
                }
                if (lo < n && hist[lo] == cv) v = 0ull;
              }
              removed += __popcll(__ballot(i >= ln && i < tot && v == 0ull));
              Lsort[i] = v;
            }
            tot -= removed;
            wave_sort_desc(Lsort, n2, lane);
            const int nl = (tot < k) ? tot : k;
            for (int i = lane; i < nl; i += 64) list[i] = Lsort[i];
            if (lane == 0) {
              *Lln = nl;
              *Lcnt = 0;
              // tau: the k-th key of this chunk's list, or what another chunk of the same user
              // has published if that is higher
              u64 t = (nl == k) ? Lsort[k - 1] : 0ull;
              if (tau_g) {
                u64* gp = tau_g + slot;
                const u64 g = (nl == k) ? atomicMax(gp, t)
                                        : __hip_atomic_load(gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (g > t) t = g;
              }
              if (t > *Ltau) {
                *Ltau = t;
                *Ltf = ord_score(uint32_t(t >> 32));
              }
            }
            wave_sync();
          }
        }
        __syncthreads();
      }
    }
  }
  __syncthreads();
  if (tid == 0) kcount[int64_t(ch) * nu + slot] = *Lln;
}

// rows of a history block: what the LDS holds beside the fixed part, a multiple of 32
int block_rows(int d) {
  const size_t per = size_t(2 * d + 1) * 4;
  const int jb = int((N1_LDS - N1_FIXED) / per) & ~31;
  return std::min(jb, N1_MAXJB);
}

}  // namespace

extern "C" {

int32_t nais_new1_forward(const nais_new1_params_t* params, const int64_t* hist,
                          int64_t hist_row_stride, const int64_t* target,
                          const int64_t* hist_region, const int64_t* target_region,
                          const float* visit_rate, int64_t b, int64_t n, float* out, void* stream) {
  if (int rc = check_params(params)) return rc;
  if (b < 0 || n < 0 || hist_row_stride < 0) return nais_internal_fail(NAIS_E_INVALID, "bad shape");
  if (b == 0) return NAIS_OK;
  if (b > (int64_t(0x7fffffff) << 2)) return nais_internal_fail(NAIS_E_UNSUPPORTED, "b too large");
  if (!target || !target_region || !out || (n > 0 && (!hist || !hist_region || !visit_rate)))
    return nais_internal_fail(NAIS_E_INVALID, "NULL pointer");
  hipLaunchKernelGGL(new1_forward_kernel, dim3((unsigned)((b + 3) / 4)), dim3(256),
                     size_t(8) * params->embed_dim * 4, reinterpret_cast<hipStream_t>(stream),
                     pack(params), hist, hist_row_stride, target, hist_region, target_region,
                     visit_rate, b, n, out);
  return nais_internal_check_launch("new1_forward_kernel");
}

int32_t nais_new1_catalog_tables(const nais_new1_params_t* params, const int64_t* region_of,
                                 float* T, float* Q, float* K, float* V, void* stream) {
  if (int rc = check_params(params)) return rc;
  if (!region_of || !T || !Q || !K || !V) return nais_internal_fail(NAIS_E_INVALID, "NULL pointer");
  const int d = params->embed_dim;
  hipLaunchKernelGGL(new1_tables_kernel, dim3((unsigned)((params->num_pois + 31) / 32)), dim3(256),
                     size_t(32) * (d + 1) * 4, reinterpret_cast<hipStream_t>(stream), pack(params),
                     region_of, T, Q, K, V);
  return nais_internal_check_launch("new1_tables_kernel");
}

size_t nais_new1_score_topk_workspace_size(const nais_new1_params_t* params, int32_t num_users,
                                           int32_t k, int32_t num_chunks) {
  if (!params || num_users <= 0 || k <= 0 || params->num_pois < 1) return 0;
  int nc;
  int64_t cpc;
  topk_chunking(params->num_pois, num_users, k, num_chunks, N1_MIN_CHUNK, &nc, &cpc);
  return topk_ws_bytes(num_users, k, nc);
}

int32_t nais_new1_score_topk(const nais_new1_params_t* params, const float* T, const float* Q,
                             const float* K, const float* V, const int64_t* indptr,
                             const int64_t* indices, const float* visit_rate, const int32_t* users,
                             int32_t num_users, int32_t k, int32_t num_chunks, uint64_t* keys,
                             int32_t* kcount, void* workspace, size_t workspace_bytes,
                             void* stream) {
  if (int rc = check_params(params)) return rc;
  if (num_users < 0 || num_chunks < 0) return nais_internal_fail(NAIS_E_INVALID, "bad shape");
  if (k < 1 || k > 256) return nais_internal_fail(NAIS_E_UNSUPPORTED, "k must be 1..256");
  if (num_users == 0) return NAIS_OK;
  if (!T || !Q || !K || !V || !indptr || !users || !keys || !kcount)   // indices / visit_rate may
    return nais_internal_fail(NAIS_E_INVALID, "NULL pointer");         // be NULL: no entries
  int nc;
  int64_t cpc;
  topk_chunking(params->num_pois, num_users, k, num_chunks, N1_MIN_CHUNK, &nc, &cpc);
  const size_t need = topk_ws_bytes(num_users, k, nc);
  if (need && (!workspace || workspace_bytes < need))
    return nais_internal_fail(NAIS_E_WORKSPACE, "workspace missing or too small");
  if (int64_t(num_users) * nc > 0x7fffffffll)
    return nais_internal_fail(NAIS_E_UNSUPPORTED, "job too large");
  const int d = params->embed_dim, JB = block_rows(d);
  const size_t lds = N1_FIXED + size_t(JB) * (2 * d + 1) * 4;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  u64* wk = (nc > 1) ? static_cast<u64*>(workspace) : reinterpret_cast<u64*>(keys);
  u64* tg = (nc > 1) ? wk + size_t(nc) * num_users * k : nullptr;
  int32_t* wc = (nc > 1) ? reinterpret_cast<int32_t*>(tg + num_users) : kcount;
  if (tg && hipMemsetAsync(tg, 0, size_t(num_users) * sizeof(u64), st) != hipSuccess)
    return nais_internal_fail(NAIS_E_HIP, "hipMemsetAsync failed");
  using kern_t = decltype(&new1_score_topk_kernel<0>);
  static const kern_t kerns[4] = {new1_score_topk_kernel<16>, new1_score_topk_kernel<32>,
                                  new1_score_topk_kernel<64>, new1_score_topk_kernel<0>};
  static bool once = [] {
    for (kern_t f : kerns)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(f),
                                hipFuncAttributeMaxDynamicSharedMemorySize, int(N1_LDS));
    return true;
  }();
  (void)once;
  const kern_t kern = kerns[(d <= 32) ? 0 : (d <= 64) ? 1 : (d <= 128) ? 2 : 3];
  hipLaunchKernelGGL(kern, dim3((unsigned)(num_users * nc)), dim3(64 * BPR_NW), lds, st, d,
                     params->num_pois, params->beta, T, Q, K, V, indptr, indices, visit_rate,
                     users, (int)num_users, (int)k, cpc, wk, wc, tg, JB);
  if (int rc = nais_internal_check_launch("new1_score_topk_kernel")) return rc;
  if (nc > 1) {
    hipLaunchKernelGGL(bpr_merge_kernel, dim3((unsigned)num_users), dim3(64), 0, st, wk, wc,
                       (int)num_users, nc, (int)k, reinterpret_cast<u64*>(keys), kcount);
    return nais_internal_check_launch("bpr_merge_kernel");
  }
  return NAIS_OK;
}

}  // extern "C"
