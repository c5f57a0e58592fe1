// nais_new2.hip -- the New2 model (model.py:927-1027) on gfx950: the batch forward and the fused
// per-user scorer + top-k (the evaluation loop of run_new.py:551-570). See include/nais.h "New2"
// and DESIGN.md "New2".
//
// New2 is New1 (nais_new1.hip; the same symbols) plus a geographic weight per (row, history item).
// With w = embed_dist[uid] (a row of R floats), b rows and n history items:
//   G[j]      = sum_c w[target_region[c]] * w[hist_region[c][j]]     (over THE BATCH, model.py:1008)
//   lambda[j] = -1 / (relu(G[j]) + 1)
//   D'[c][j]  = distflat[c * n + j]     (dist arrives as [n, b] and is RESHAPED to [b, n])
//   geo[c][j] = expf(lambda[j] * D'[c][j])                           (not masked)
//   pred_c    = sum_j (e_cj / S_c^beta + geo[c][j]) * (V_j . t_c)  +  t_c . sum_j r_j h_j
// In evaluation the batch is the user's complement in ascending POI id and every row shares the
// history, so G[j] = w[region(hist_j)] * sigma_u with sigma_u = sum over the candidates of
// w[region(c)], one scalar per user formed from per-region counts; and row c (the c-th candidate
// by position) pairs history item (c n + j) div b with candidate POSITION (c n + j) mod b.
//
// The scorer is New1's (one workgroup = one user x one column chunk, K scrambled and V rows in
// LDS, two v_mfma_f32_32x32x2_f32 chains per 32-row history tile) with a third running sum per
// lane, Gs += geo * C2 from the same V.t accumulator, and lambda[j] per LDS row. New1's file is
// left as it is: sharing the body through a header templated on the epilogue would have to
// reproduce its register allocation (154 / 219 / 256 VGPRs), which the fp64 temporaries of this
// epilogue do not allow to take for granted.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "nais_geo.h"
#include "nais_internal.h"
#include "nais_topk_dev.h"

typedef float floatx16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int N2_SUPER = 8;                 // steps per superstep of the j-tiled route
constexpr int N2_MAXJB = 2048;              // rows of a history block at most
constexpr int64_t N2_MIN_CHUNK = 2048;      // columns per chunk at least (the warm-up of tau)
// LDS before the history block: buffer, sort space, tau (padded), 7 ints + tau's score + sigma
// (padded to 48 B), g, three parked sums per lane and step
constexpr size_t N2_FIXED = size_t(BPR_BUF + BPR_SORT + 2) * 8 + 48 + 256 * 4 +
                            size_t(N2_SUPER) * 64 * BPR_NW * 3 * 4;
constexpr size_t N2_LDS = 160 * 1024;
constexpr double N2_DIAMETER_KM = 2.0 * 6371.0088;   // haversine: 2 * mean radius, kilometres

__device__ __forceinline__ int crow(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

struct NP2 {
  int d;
  int64_t P, R, U;
  float beta;
  const float *E, *Er, *Wq, *Wk, *Wv, *Wd;
};

int check_params(const nais_new2_params_t* q2) {
  if (!q2) return nais_internal_fail(NAIS_E_INVALID, "NULL params");
  const nais_new1_params_t* q = &q2->base;
  if (q->embed_dim < 2 || q->embed_dim > 256 || (q->embed_dim & 1))
    return nais_internal_fail(NAIS_E_UNSUPPORTED, "New2 embed_dim must be even, 2..256");
  if (q->hidden != q->embed_dim)
    return nais_internal_fail(NAIS_E_UNSUPPORTED,
                              "New2 hidden must equal embed_dim (the reshape of model.py:996)");
  if (q->num_pois < 1 || q->num_regions < 1 || q2->num_users < 1)
    return nais_internal_fail(NAIS_E_INVALID, "bad shape");
  if (q->num_pois >= (int64_t(1) << 24))
    return nais_internal_fail(NAIS_E_UNSUPPORTED, "New2 num_pois must be below 2^24");
  if (q->num_regions >= (int64_t(1) << 31))
    return nais_internal_fail(NAIS_E_UNSUPPORTED, "New2 num_regions must be below 2^31");
  if (!q->embed_target || !q->embed_region || !q->attn_q || !q->attn_k || !q->attn_v ||
      !q2->embed_dist)
    return nais_internal_fail(NAIS_E_INVALID, "NULL parameter pointer");
  return NAIS_OK;
}

NP2 pack(const nais_new2_params_t* q2) {
  const nais_new1_params_t* q = &q2->base;
  return NP2{q->embed_dim, q->num_pois,     q->num_regions, q2->num_users, q->beta,      q->embed_target,
             q->embed_region, q->attn_q,    q->attn_k,      q->attn_v,     q2->embed_dist};
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

__device__ __forceinline__ float lambda_of(float G) { return -1.f / (nais_relu(G) + 1.f); }

// ---- lambda[j] of a batch: one workgroup per history column j. Lane t adds the rows c = t, t + 256,
// ... in ascending order, then a fixed tree: same input, same bits.
__global__ __launch_bounds__(256) void new2_lambda_kernel(
    const float* __restrict__ Wd, int64_t U, int64_t R, int64_t uid, const int64_t* __restrict__ hreg,
    int64_t hs, const int64_t* __restrict__ treg, int64_t b, float* __restrict__ lam) {
  __shared__ float red[256];
  const int tid = threadIdx.x;
  const int64_t j = blockIdx.x;
  float s = 0.f;
  if (uid >= 0 && uid < U) {
    const float* __restrict__ w = Wd + uid * R;
    for (int64_t c = tid; c < b; c += 256) {
      const int64_t tr = treg[c], hr = hreg[c * hs + j];
      const float tau = (tr >= 0 && tr < R) ? w[tr] : __builtin_nanf("");
      const float om = (hr >= 0 && hr < R) ? w[hr] : __builtin_nanf("");
      s = fmaf(tau, om, s);
    }
  } else {
    s = __builtin_nanf("");
  }
  red[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) lam[j] = lambda_of(red[0]);
}

// ---- forward: new1_forward_kernel with the geo weight added to the attention weight
__global__ __launch_bounds__(256) void new2_forward_kernel(
    NP2 p, const int64_t* __restrict__ hist, int64_t hs, const int64_t* __restrict__ target,
    const int64_t* __restrict__ hreg, const int64_t* __restrict__ treg,
    const float* __restrict__ vr, const float* __restrict__ dist, const float* __restrict__ lam,
    int64_t uid, int64_t b, int64_t n, float* __restrict__ out) {
  extern __shared__ float new2_fwd_lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int d = p.d, half = d >> 1;
  const int64_t row = int64_t(blockIdx.x) * 4 + wave;
  if (row >= b) return;   // whole waves leave; the rest of the kernel has no workgroup barrier
  float* Lt = new2_fwd_lds + wave * 2 * d;
  float* Lq = Lt + d;
  const int64_t* __restrict__ hrow = hist + row * hs;
  const int64_t* __restrict__ rrow = hreg + row * hs;
  const int64_t c = target[row], tr = treg[row];
  bool ok = c >= 0 && c < p.P && tr >= 0 && tr < p.R && uid >= 0 && uid < p.U;
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
    // attn_weights + geo_weights (model.py:1009); the distance block read flat at c * n + j
    const float w = expa(j) / pw + expf(lam[j] * dist[row * n + j]), r = vr[j];
    for (int k = 0; k < d; ++k) {
      float v = 0.f;
      for (int m = 0; m < d; ++m) v = fmaf(h(j, m), p.Wv[k * d + m], v);
      acc = fmaf(fmaf(w, v, r * h(j, k)), Lt[k], acc);
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) out[row] = sigmoidf((n == 0) ? 0.f : acc);
}

// ---- per-call tables of the scorer: POIs per region, and (lat, lng in radians, cos lat) per POI
__global__ __launch_bounds__(256) void new2_region_count_kernel(
    const int64_t* __restrict__ region_of, int64_t P, int64_t R, int32_t* __restrict__ cnt) {
  const int64_t p = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (p >= P) return;
  const int64_t rg = region_of[p];
  if (rg >= 0 && rg < R) atomicAdd(cnt + rg, 1);   // integers: the order does not matter
}

struct GP {
  double lat, lng, cl;
};

__global__ __launch_bounds__(256) void new2_geo_table_kernel(const double* __restrict__ coords,
                                                             int64_t P, double* __restrict__ tab) {
  const int64_t p = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (p >= P) return;
  const double lat = __dmul_rn(coords[2 * p], kD2R), lng = __dmul_rn(coords[2 * p + 1], kD2R);
  tab[3 * p] = lat;
  tab[3 * p + 1] = lng;
  tab[3 * p + 2] = cos(lat);
}

__device__ __forceinline__ GP geo_row(const double* __restrict__ tab, int64_t p) {
  return GP{tab[3 * p], tab[3 * p + 1], tab[3 * p + 2]};
}

// the haversine package's formula in its operation order, float64, kilometres, rounded to float32:
//   d = sin(dlat / 2)^2 + cos(lat1) cos(lat2) sin(dlng / 2)^2;  2 R asin(sqrt(d))
__device__ __forceinline__ float haversine_km(const GP& a, const GP& b) {
  const double sl = sin(__dmul_rn(__dsub_rn(b.lat, a.lat), 0.5));
  const double sg = sin(__dmul_rn(__dsub_rn(b.lng, a.lng), 0.5));
  const double dd =
      __dadd_rn(__dmul_rn(sl, sl), __dmul_rn(__dmul_rn(a.cl, b.cl), __dmul_rn(sg, sg)));
  return float(__dmul_rn(N2_DIAMETER_KM, asin(sqrt(dd))));
}

// ---- the scorer. NPR: k pairs a lane keeps of q_c and t_c (d <= 2 * NPR); 0: read in the loop.
template <int NPR>
__global__ __launch_bounds__(64 * BPR_NW) void new2_score_topk_kernel(
    int d, int64_t P, int64_t R, int64_t U, float beta, const float* __restrict__ Wd,
    const float* __restrict__ T, const float* __restrict__ Q, const float* __restrict__ K,
    const float* __restrict__ V, const int64_t* __restrict__ region_of,
    const int32_t* __restrict__ rcount, const double* __restrict__ gtab,
    const float* __restrict__ dist_mat, const int64_t* __restrict__ indptr,
    const int64_t* __restrict__ indices, const float* __restrict__ vr,
    const int32_t* __restrict__ users, int nu, int k, int64_t cpc, u64* __restrict__ keys,
    int32_t* __restrict__ kcount, u64* __restrict__ tau_g, int JB) {
  extern __shared__ u64 new2_lds[];
  u64* Lbuf = new2_lds;                                  // [BPR_BUF]
  u64* Lsort = Lbuf + BPR_BUF;                           // [BPR_SORT]
  u64* Ltau = Lsort + BPR_SORT;                          // [1] (+ 1 pad)
  int* Lcnt = reinterpret_cast<int*>(Ltau + 2);          // keys in the buffer
  int* Lln = Lcnt + 1;                                   // keys in the list
  int* Lneed = Lln + 1;                                  // [4] (3 used) "the buffer wants compacting"
  float* Ltf = reinterpret_cast<float*>(Lneed + 4);      // the score in tau, as a float (+ 1 pad)
  float* Lsig = Ltf + 2;                                 // sigma_u (+ 3 pad)
  float* Lg = Lsig + 4;                                  // [256] g = sum_j r_j h_j
  float* Lacc = Lg + 256;                                // [N2_SUPER][256][3] parked running sums
  float* Lk = Lacc + N2_SUPER * 64 * BPR_NW * 3;         // [d][pk]
  float* Lv = Lk + size_t(d) * JB;                       // [JB][d + 1]
  float* Ll = Lv + size_t(JB) * (d + 1);                 // [JB] lambda of the block's rows

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
  const int b = (int(P) - n > 1) ? int(P) - n : 1;       // candidates of the user (1: none, unused)
  const bool many = n > b;                               // a row's positions wrap more than once
  const float* __restrict__ wrow = (u >= 0 && u < U) ? Wd + u * R : nullptr;
  auto omega = [&](int64_t rg) {   // embed_dist[u][rg]; NaN for a user or region outside the table
    return (wrow && rg >= 0 && rg < R) ? wrow[rg] : __builtin_nanf("");
  };

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
  {
    // sigma_u = sum over the candidates of w[region]: per region (POIs - history POIs) * w, in
    // float64 (every product is exact), lane t over r = t, t + 256, ..., then a fixed tree
    double* Lred = reinterpret_cast<double*>(Lsort);
    double part = 0.0;
    for (int64_t r = tid; r < R; r += 64 * BPR_NW)
      part += double(rcount[r]) * double(wrow ? wrow[r] : __builtin_nanf(""));
    for (int j = tid; j < n; j += 64 * BPR_NW) part -= double(omega(region_of[hist[j]]));
    Lred[tid] = part;
    __syncthreads();
    for (int o = 32 * BPR_NW; o > 0; o >>= 1) {
      if (tid < o) Lred[tid] += Lred[tid + o];
      __syncthreads();
    }
    if (tid == 0) *Lsig = float(Lred[0]);
  }

  const int nblk = (n > JB) ? (n + JB - 1) / JB : 1;
  const int64_t ntiles = (c_end - c_begin + BPR_STEP - 1) / BPR_STEP;
  const int64_t sps = (nblk > 1) ? N2_SUPER : ((ntiles > 0) ? ntiles : 1);
  u64* list = keys + (int64_t(ch) * nu + slot) * k;

  for (int64_t s0 = 0; s0 < ntiles; s0 += sps) {
    const int64_t s1 = (s0 + sps < ntiles) ? s0 + sps : ntiles;
    for (int blk = 0; blk < nblk; ++blk) {
      const int jb0 = blk * JB;
      const int jw = (n - jb0 < JB) ? n - jb0 : JB;      // rows of this block (0 for no history)
      const int jwp = (jw + 31) & ~31;                   // <= pk
      if (nblk > 1 || s0 == 0) {
        __syncthreads();   // every wave is done with the previous block; sigma_u is written
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
        const float sig = *Lsig;
        for (int jj = tid; jj < jwp; jj += 64 * BPR_NW)
          Ll[jj] = (jj < jw) ? lambda_of(omega(region_of[hist[jb0 + jj]]) * sig) : 0.f;
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
        float S = 0.f, N = 0.f, Gs = 0.f;
        float* park = Lacc + (size_t(step - s0) * 64 * BPR_NW + tid) * 3;
        if (blk > 0) {
          S = park[0];
          N = park[1];
          Gs = park[2];
        }
        // The candidate's row of the reshaped distance block. pos: its position among the user's
        // candidates (a history POI or a padding lane takes 0: its score is dropped later); the
        // row starts at flat index pos * n = i0 * b + m0.
        int i0 = 0, m0 = 0, pa = 0, pb = 0;
        GP ga{0.0, 0.0, 0.0}, gb{0.0, 0.0, 0.0};
        if (jw > 0) {
          int lo = 0, hi = n;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (hist[mid] < cc) lo = mid + 1; else hi = mid;
          }
          const int64_t pos = (lo < n && hist[lo] == cc) ? 0 : cc - lo;
          const int64_t f0 = pos * n;
          i0 = int(f0 / b);
          m0 = int(f0 - int64_t(i0) * b);
          i0 = (i0 < n) ? i0 : n - 1;
          pa = int(hist[i0]);
          pb = int(hist[(i0 + 1 < n) ? i0 + 1 : n - 1]);
          if (gtab) {
            ga = geo_row(gtab, pa);
            gb = geo_row(gtab, pb);
          }
        }
        int mprev = 0x7fffffff, below = 0;   // below = #{t : hist_t - t <= mprev}
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
          // The geo term of the same rows, one at a time (the float64 distance is long code; r
          // is wave-uniform, so C2[r] is a register index, not memory). j ascends with r, so the
          // position m ascends too, except where it wraps past b.
#pragma unroll 1
          for (int r = 0; r < 16; ++r) {
            const int jl = jt + crow(r, hh);
            if (jl >= jw) continue;
            int m = m0 + jb0 + jl, i = i0;
            if (many) {
              if (m >= b) {
                const int q = m / b;
                m -= q * b;
                i += q;
              }
            } else if (m >= b) {
              m -= b;
              i += 1;
            }
            // position -> POI id: m + #{t : hist_t - t <= m} on the sorted history
            if (m < mprev) {
              int lo = 0, hi = n;
              while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (int(hist[mid]) - mid <= m) lo = mid + 1; else hi = mid;
              }
              below = lo;
            } else {
              while (below < n && int(hist[below]) - below <= m) ++below;
            }
            mprev = m;
            int64_t id = int64_t(m) + below;
            id = (id < P) ? id : P - 1;
            int ph = (i == i0) ? pa : pb;
            if (many) ph = int(hist[(i < n) ? i : n - 1]);
            float D;
            if (gtab) {
              GP gh = (i == i0) ? ga : gb;
              if (many) gh = geo_row(gtab, ph);
              D = haversine_km(gh, geo_row(gtab, id));
            } else {
              D = dist_mat[int64_t(ph) * P + id];
            }
            Gs = fmaf(expf(Ll[jl] * D), C2[r], Gs);
          }
        }
        if (!last_blk) {   // workgroup-uniform
          park[0] = S;
          park[1] = N;
          park[2] = Gs;
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
        Gs += __shfl_xor(Gs, 32);
        gd += __shfl_xor(gd, 32);
        const float pred = (n == 0) ? 0.f : N / powf(S, beta) + Gs + gd;
        const float score = bpr_canon(sigmoidf(pred));
        const int ph3 = int(step % 3);
        // one compare per score: below tau's score (a NaN on either side passes) it is no
        // survivor; else the whole key against tau
        if (hh == 0 && c < c_end && !(score < *Ltf)) {
          const u64 key = (u64(ord_bits(score)) << 32) | u64(0xFFFFFFFFu - uint32_t(c));
          if (key > *Ltau) {
            const int pos = atomicAdd(Lcnt, 1);
            if (pos < BPR_BUF) Lbuf[pos] = key;   // always true: <= BPR_STEP keys per step
            if (pos >= BPR_TRIG) Lneed[ph3] = 1;
          }
        }
        __syncthreads();

        // Most steps compact nothing and have this one barrier. The flag of step t + 2 is cleared
        // here: it was last read in step t - 1, and is next set after the barrier of step t + 1.
        const bool last = step + 1 == ntiles;
        const bool need = Lneed[ph3] != 0 || last;
        if (tid == 0) Lneed[(ph3 + 2) % 3] = 0;
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
  const size_t per = size_t(2 * d + 2) * 4;
  const int jb = int((N2_LDS - N2_FIXED) / per) & ~31;
  return std::min(jb, N2_MAXJB);
}

size_t up16(size_t x) { return (x + 15) & ~size_t(15); }

// workspace: the chunked top-k part, the POIs per region, the per-POI coordinate table
size_t ws_bytes(const nais_new2_params_t* q, int nu, int k, int nc) {
  return up16(topk_ws_bytes(nu, k, nc)) + up16(size_t(q->base.num_regions) * sizeof(int32_t)) +
         size_t(q->base.num_pois) * 3 * sizeof(double);
}

}  // namespace

extern "C" {

int32_t nais_new2_forward(const nais_new2_params_t* params, const int64_t* hist,
                          int64_t hist_row_stride, const int64_t* target,
                          const int64_t* hist_region, const int64_t* target_region,
                          const float* visit_rate, const float* dist, int64_t uid, int64_t b,
                          int64_t n, float* lambda_work, float* out, void* stream) {
  if (int rc = check_params(params)) return rc;
  if (b < 0 || n < 0 || hist_row_stride < 0) return nais_internal_fail(NAIS_E_INVALID, "bad shape");
  if (b == 0) return NAIS_OK;
  if (b > (int64_t(0x7fffffff) << 2)) return nais_internal_fail(NAIS_E_UNSUPPORTED, "b too large");
  if (n > 0x7fffffffll) return nais_internal_fail(NAIS_E_UNSUPPORTED, "n too large");
  if (!target || !target_region || !out ||
      (n > 0 && (!hist || !hist_region || !visit_rate || !dist || !lambda_work)))
    return nais_internal_fail(NAIS_E_INVALID, "NULL pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const NP2 p = pack(params);
  if (n > 0) {
    hipLaunchKernelGGL(new2_lambda_kernel, dim3((unsigned)n), dim3(256), 0, st, p.Wd, p.U, p.R, uid,
                       hist_region, hist_row_stride, target_region, b, lambda_work);
    if (int rc = nais_internal_check_launch("new2_lambda_kernel")) return rc;
  }
  hipLaunchKernelGGL(new2_forward_kernel, dim3((unsigned)((b + 3) / 4)), dim3(256),
                     size_t(8) * p.d * 4, st, p, hist, hist_row_stride, target, hist_region,
                     target_region, visit_rate, dist, lambda_work, uid, b, n, out);
  return nais_internal_check_launch("new2_forward_kernel");
}

size_t nais_new2_score_topk_workspace_size(const nais_new2_params_t* params, int32_t num_users,
                                           int32_t k, int32_t num_chunks) {
  if (!params || num_users <= 0 || k <= 0 || params->base.num_pois < 1 ||
      params->base.num_regions < 1)
    return 0;
  int nc;
  int64_t cpc;
  topk_chunking(params->base.num_pois, num_users, k, num_chunks, N2_MIN_CHUNK, &nc, &cpc);
  return ws_bytes(params, num_users, k, nc);
}

int32_t nais_new2_score_topk(const nais_new2_params_t* params, const float* T, const float* Q,
                             const float* K, const float* V, const int64_t* region_of,
                             const int64_t* indptr, const int64_t* indices,
                             const float* visit_rate, const double* coords, const float* dist_mat,
                             const int32_t* users, int32_t num_users, int32_t k,
                             int32_t num_chunks, uint64_t* keys, int32_t* kcount, void* workspace,
                             size_t workspace_bytes, void* stream) {
  if (int rc = check_params(params)) return rc;
  if (num_users < 0 || num_chunks < 0) return nais_internal_fail(NAIS_E_INVALID, "bad shape");
  if (k < 1 || k > 256) return nais_internal_fail(NAIS_E_UNSUPPORTED, "k must be 1..256");
  if (num_users == 0) return NAIS_OK;
  if (!T || !Q || !K || !V || !region_of || !indptr || !users || !keys || !kcount)
    return nais_internal_fail(NAIS_E_INVALID, "NULL pointer");   // indices / visit_rate may be NULL
  if (!coords == !dist_mat)
    return nais_internal_fail(NAIS_E_INVALID, "give exactly one of coords and dist_mat");
  const int64_t P = params->base.num_pois, R = params->base.num_regions;
  int nc;
  int64_t cpc;
  topk_chunking(P, num_users, k, num_chunks, N2_MIN_CHUNK, &nc, &cpc);
  if (!workspace || workspace_bytes < ws_bytes(params, num_users, k, nc))
    return nais_internal_fail(NAIS_E_WORKSPACE, "workspace missing or too small");
  if (int64_t(num_users) * nc > 0x7fffffffll)
    return nais_internal_fail(NAIS_E_UNSUPPORTED, "job too large");
  const int d = params->base.embed_dim, JB = block_rows(d);
  const size_t lds = N2_FIXED + size_t(JB) * (2 * d + 2) * 4;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* wsp = static_cast<char*>(workspace);
  int32_t* rcount = reinterpret_cast<int32_t*>(wsp + up16(topk_ws_bytes(num_users, k, nc)));
  double* gtab = reinterpret_cast<double*>(reinterpret_cast<char*>(rcount) +
                                           up16(size_t(R) * sizeof(int32_t)));
  u64* wk = (nc > 1) ? reinterpret_cast<u64*>(wsp) : reinterpret_cast<u64*>(keys);
  u64* tg = (nc > 1) ? wk + size_t(nc) * num_users * k : nullptr;
  int32_t* wc = (nc > 1) ? reinterpret_cast<int32_t*>(tg + num_users) : kcount;
  if (tg && hipMemsetAsync(tg, 0, size_t(num_users) * sizeof(u64), st) != hipSuccess)
    return nais_internal_fail(NAIS_E_HIP, "hipMemsetAsync failed");
  if (hipMemsetAsync(rcount, 0, size_t(R) * sizeof(int32_t), st) != hipSuccess)
    return nais_internal_fail(NAIS_E_HIP, "hipMemsetAsync failed");
  hipLaunchKernelGGL(new2_region_count_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st,
                     region_of, P, R, rcount);
  if (int rc = nais_internal_check_launch("new2_region_count_kernel")) return rc;
  if (coords) {
    hipLaunchKernelGGL(new2_geo_table_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st,
                       coords, P, gtab);
    if (int rc = nais_internal_check_launch("new2_geo_table_kernel")) return rc;
  }
  using kern_t = decltype(&new2_score_topk_kernel<0>);
  static const kern_t kerns[4] = {new2_score_topk_kernel<16>, new2_score_topk_kernel<32>,
                                  new2_score_topk_kernel<64>, new2_score_topk_kernel<0>};
  static bool once = [] {
    for (kern_t f : kerns)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(f),
                                hipFuncAttributeMaxDynamicSharedMemorySize, int(N2_LDS));
    return true;
  }();
  (void)once;
  const kern_t kern = kerns[(d <= 32) ? 0 : (d <= 64) ? 1 : (d <= 128) ? 2 : 3];
  hipLaunchKernelGGL(kern, dim3((unsigned)(num_users * nc)), dim3(64 * BPR_NW), lds, st, d, P, R,
                     params->num_users, params->base.beta, params->embed_dist, T, Q, K, V,
                     region_of, rcount, coords ? gtab : nullptr, dist_mat, indptr, indices,
                     visit_rate, users, (int)num_users, (int)k, cpc, wk, wc, tg, JB);
  if (int rc = nais_internal_check_launch("new2_score_topk_kernel")) return rc;
  if (nc > 1) {
    hipLaunchKernelGGL(bpr_merge_kernel, dim3((unsigned)num_users), dim3(64), 0, st, wk, wc,
                       (int)num_users, nc, (int)k, reinterpret_cast<u64*>(keys), kcount);
    return nais_internal_check_launch("bpr_merge_kernel");
  }
  return NAIS_OK;
}

}  // extern "C"
