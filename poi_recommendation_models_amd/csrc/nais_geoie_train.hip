// nais_geoie_train.hip -- GeoIE training on gfx950: the device-side get_GeoIE_batch
// (batches.py:204-242) and the fused step forward + loss_function + backward + SGD
// (run.py:705-715, model.py:785-828). See include/nais.h "GeoIE training" for the arithmetic.
//
// One batch is one user: b target rows that all share ONE history hist[h]. With F = [f_ij]
// ([b, h], f = a * d ** b) and Gr^T ([h, D]: Gr^T[j][e] = flat[e*h + j], the scramble of
// model.py:798) the step is two skinny exact-fp32 MFMA products around an elementwise pass:
//
//   geoie_step_fwd_kernel   one workgroup per 32 target rows. T = F . Gr^T ([32, D] per workgroup;
//                           v_mfma_f32_32x32x2_f32 over j, the history staged in LDS chunks of
//                           GT_JC rows so any h works, one or two 32-column tiles of T per wave).
//                           Then per row y = T . GeoSusceptibility[c] / h, the preference dot,
//                           p, the loss term and delta; T, F, delta and the workgroup's partial
//                           of dUserPreference go to the workspace. Nothing is updated here.
//   geoie_step_geo_kernel   dflat = (diag(delta / h) Hs)^T . F ([D, b] x [b, h]) in 32 x 32 tiles,
//                           the K = b extent split over the workgroup's 8 waves and summed in LDS
//                           in wave order. Flat position m = e*h + j is GeoInfluence[hist[m / D]]
//                           [m % D]: history entries are distinct, so every position is one
//                           element and is updated in place without atomics (GeoInfluence is read
//                           only by the forward kernel, which has finished).
//   geoie_step_rows_kernel  one wave per target row: dGeoSusceptibility[c] = (delta / h) T[i],
//                           dPoiPreference[c] = delta * UserPreference[u] (the copy the forward
//                           kernel saved), and one wave for the user row (the partials summed in
//                           workgroup order). Runs after the geo kernel, which reads Hs.
//   sgd_rows_kernel         weight_decay != 0 only: p -= lr * (weight_decay * p) for the rows the
//                           step did not touch (stamp != tag), so no row moves twice.
//
// The K extents are rounded up to even and the tile edges to 32; that padding is zero in both
// operands and is added AFTER the scramble (the scramble indexes the unpadded h*D floats).
// Repeated targets, repeated history entries and ids outside [0, P) are detected in the forward
// kernel (atomicExch on the [P] stamp arrays, the step's tag) and set *err; while *err is set no
// table is written, so a repeat is never applied half-summed.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "nais_geo.h"
#include "nais_geo_cr.h"
#include "nais_internal.h"

typedef float floatx16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int GT_JC = 64;      // history rows per LDS chunk of the forward kernel
constexpr int GT_FP = GT_JC + 1;   // pitch of the F tile: lanes over rows read distinct banks
constexpr int GT_KW = 8;       // waves of the geo kernel (they split K = b)
constexpr int GT_BR = 16;      // target rows per workgroup of the batch distance kernel

struct TP {
  int D;
  int64_t P;
  float* U;
  float* Pp;
  float* G;
  float* H;
};

// workspace carve-up (floats), shared by the three kernels
struct WS {
  float* F;        // [b, h]
  float* T;        // [b, D]
  float* delta;    // [b]
  float* dh;       // [b]   delta / h
  float* upart;    // [ceil(b / 32), D]
  float* uold;     // [D]
  int32_t* cidx;   // [b]   target ids, clamped to [0, P)
};

size_t ws_floats(int64_t b, int64_t h, int64_t D) {
  const int64_t nblk = (b + 31) / 32;
  return size_t(b * h + b * D + 3 * b + nblk * D + D + 16);
}

WS carve(void* w, int64_t b, int64_t h, int64_t D) {
  const int64_t nblk = (b + 31) / 32;
  WS s;
  s.F = static_cast<float*>(w);
  s.T = s.F + b * h;
  s.delta = s.T + b * D;
  s.dh = s.delta + b;
  s.upart = s.dh + b;
  s.uold = s.upart + nblk * D;
  s.cidx = reinterpret_cast<int32_t*>(s.uold + D);
  return s;
}

// row of the 32x32 accumulator held in register r by lane half hh
__device__ __forceinline__ int crow(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

__device__ __forceinline__ double clamp_dist(double d) {   // run.py:44, as nais_geoie_table
  const double lo = (d > 0.01) ? d : 0.01;
  return (100.0 < lo) ? 100.0 : lo;
}

// make_geo / ref_dist of nais_geo.h (the same operations in the same order) with the sin, cos and
// acos of nais_geo_cr.h: the batch's distances feed the model as the reference's dist_mat does,
// and between POIs closer than 0.3 km a last-bit difference moves them by up to a hundred
// float32 ulps. The products and sums are plain operators with contraction switched off:
// __dmul_rn / __dadd_rn are inline x * y and x + y of a header compiled with contraction on,
// which the compiler fuses (cosv's last product into its sum) wherever they are inlined.
__device__ __forceinline__ Geo make_geo_cr(double lat, double lng) {
  NAIS_CR_NO_CONTRACT
  const double phi = (90.0 - lat) * kD2R;
  nais_geo_cr::DD s, c;
  if (fabs(phi) < 1e5) {
    nais_geo_cr::sincos_dd(phi, &s, &c, 3);
  } else {
    s.h = sin(phi);
    c.h = cos(phi);
  }
  return Geo{lat, lng, s.h, c.h, lng * kD2R};
}

__device__ __forceinline__ double ref_dist_cr(const Geo& p1, const Geo& p2) {
  NAIS_CR_NO_CONTRACT
  if (fabs(p1.lat - p2.lat) < 1e-6 && fabs(p1.lng - p2.lng) < 1e-6) return 0.0;
  const double t = (p1.sphi * p2.sphi) * nais_geo_cr::cr_cos(p1.theta - p2.theta);
  const double cosv = t + p1.cphi * p2.cphi;
  return nais_geo_cr::cr_acos(cosv) * 6371.0;
}

__device__ __forceinline__ float sigmoidf(float s) { return 1.0f / (1.0f + expf(-s)); }

// torch.optim.SGD without momentum: g' = g + weight_decay * p; p -= lr * g'
__device__ __forceinline__ float sgd_elem(float p, float g, float lr, float wd) {
  const float gg = (wd != 0.f) ? fmaf(wd, p, g) : g;
  return fmaf(-lr, gg, p);
}

// ---------------------------------------------------------------------------------------------
// batch builder, second half: freq and distances for the ids nais_make_train_batch drew
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void geoie_batch_fill_kernel(
    const int64_t* __restrict__ indptr, const double* __restrict__ data, int64_t user, int64_t h,
    int64_t b, int ng, int64_t P, const double* __restrict__ coords,
    const double* __restrict__ dist_mat, const int64_t* __restrict__ hist,
    const int64_t* __restrict__ target, int64_t* __restrict__ freq, float* __restrict__ dist,
    int64_t ld, int64_t nct) {
  __shared__ Geo Lg[GT_BR];
  __shared__ int64_t Lt[GT_BR];
  const int tid = threadIdx.x;
  const int64_t ct = int64_t(blockIdx.x) % nct, r0 = (int64_t(blockIdx.x) / nct) * GT_BR;
  if (tid < GT_BR && r0 + tid < b) {
    const int64_t i = r0 + tid;
    int64_t t = target[i];
    if (t < 0 || t >= P) t = 0;   // only after an h mismatch (*err is set): keep the reads in range
    Lt[tid] = t;
    if (coords) Lg[tid] = make_geo_cr(coords[2 * t], coords[2 * t + 1]);
    // freq is attached by CSR position, not by POI (batches.py:238-239)
    if (ct == 0) freq[i] = int64_t(data[indptr[user] + i / (1 + ng)]);
  }
  __syncthreads();
  const int64_t j = ct * 256 + tid;
  if (j >= h) return;
  int64_t hj = hist[j];
  if (hj < 0 || hj >= P) hj = 0;
  const int nr = (b - r0 < GT_BR) ? int(b - r0) : GT_BR;
  if (coords) {
    const Geo gh = make_geo_cr(coords[2 * hj], coords[2 * hj + 1]);
    for (int i = 0; i < nr; ++i)   // dist_mat[target][hist] = dist(coo[target], coo[hist]), run.py:44
      dist[(r0 + i) * ld + j] = float(clamp_dist(ref_dist_cr(Lg[i], gh)));
  } else {
    for (int i = 0; i < nr; ++i) dist[(r0 + i) * ld + j] = float(dist_mat[Lt[i] * P + hj]);
  }
}

// ---------------------------------------------------------------------------------------------
// forward, loss and delta
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void geoie_step_fwd_kernel(
    TP p, int64_t user, const int64_t* __restrict__ hist, uint32_t h,
    const int64_t* __restrict__ target, const float* __restrict__ labels,
    const int64_t* __restrict__ freq, int64_t b, const float* __restrict__ dist, int64_t dist_ld,
    float a, float pw, int32_t* __restrict__ st_t, int32_t* __restrict__ st_h, int32_t tag, WS w,
    float* __restrict__ loss_sum, int32_t* __restrict__ bad_rows, int32_t* __restrict__ err,
    float* __restrict__ pred, int pitch, int DP32) {
  extern __shared__ float gt_lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 31, hh = lane >> 5;
  const int D = p.D;
  float* Lg = gt_lds;                               // [GT_JC][pitch]; later the T tile [32][pitch]
  float* Lf = Lg + GT_JC * pitch;                   // [32][GT_FP]
  float* Ld = Lf + 32 * GT_FP;                      // [32] delta
  int* Lc = reinterpret_cast<int*>(Ld + 32);        // [32] clamped target ids
  const int64_t i0 = int64_t(blockIdx.x) * 32;
  const float* __restrict__ Gp = p.G;

  // ids: range and repeats (the history once, by workgroup 0)
  if (tid < 32) {
    const int64_t i = i0 + tid;
    int c = 0;
    if (i < b) {
      const int64_t t = target[i];
      if (t < 0 || t >= p.P) atomicOr(err, 2);
      else {
        c = int(t);
        if (atomicExch(st_t + t, tag) == tag) atomicOr(err, 1);
      }
      w.cidx[i] = c;
    }
    Lc[tid] = c;
  }
  if (blockIdx.x == 0) {
    for (uint32_t j = tid; j < h; j += 256) {
      const int64_t t = hist[j];
      if (t < 0 || t >= p.P) atomicOr(err, 2);
      else if (atomicExch(st_h + t, tag) == tag) atomicOr(err, 1);
    }
    for (int e = tid; e < D; e += 256) w.uold[e] = p.U[user * D + e];
  }

  floatx16 acc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  for (uint32_t jc0 = 0; jc0 < h; jc0 += GT_JC) {
    __syncthreads();   // the previous chunk is consumed
    const int nj = (h - jc0 < uint32_t(GT_JC)) ? int(h - jc0) : GT_JC;
    const int njp = (nj + 31) & ~31;                  // 32 or 64
    const int sh = (njp == 32) ? 5 : 6;
    // Gr^T rows [jc0, jc0 + nj): consecutive threads take consecutive j, i.e. consecutive
    // elements m = e*h + j of the flat gather; zero past nj and past column D
    for (int idx = tid; idx < njp * DP32; idx += 256) {
      const int e = idx >> sh, jj = idx & (njp - 1);
      float v = 0.f;
      if (jj < nj && e < D) {
        const uint32_t m = uint32_t(e) * h + jc0 + uint32_t(jj);
        const uint32_t r = m / uint32_t(D);
        int64_t hr = hist[r];
        if (hr < 0 || hr >= p.P) hr = 0;
        v = Gp[hr * D + (m - r * uint32_t(D))];
      }
      Lg[jj * pitch + e] = v;
    }
    // F tile [32][njp] = a * d ** b (model.py:799), zero past row b and past nj; kept for the
    // geo kernel
    for (int idx = tid; idx < 32 * njp; idx += 256) {
      const int ii = idx >> sh, jj = idx & (njp - 1);
      float v = 0.f;
      if (i0 + ii < b && jj < nj) {
        v = a * powf(dist[(i0 + ii) * dist_ld + jc0 + jj], pw);
        w.F[(i0 + ii) * int64_t(h) + jc0 + jj] = v;
      }
      Lf[ii * GT_FP + jj] = v;
    }
    __syncthreads();
    const int kend = (nj + 1) & ~1;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int e0 = (wave + 4 * t) * 32;               // wave-uniform
      if (e0 < DP32) {
        const float* ap = Lf + n * GT_FP + hh;
        const float* bp = Lg + hh * pitch + e0 + n;
        for (int k0 = 0; k0 < kend; k0 += 2)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[k0], bp[k0 * pitch], acc[t], 0, 0, 0);
      }
    }
  }
  __syncthreads();   // every wave is done with the last chunk: Lg becomes the T tile
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int e0 = (wave + 4 * t) * 32;
    if (e0 < DP32) {
#pragma unroll
      for (int r = 0; r < 16; ++r) Lg[crow(r, hh) * pitch + e0 + n] = acc[t][r];
    }
  }
  __syncthreads();
  for (int idx = tid; idx < 32 * D; idx += 256) {
    const int ii = idx / D, e = idx - ii * D;
    if (i0 + ii < b) w.T[(i0 + ii) * D + e] = Lg[ii * pitch + e];
  }

  // per row: eight lanes share the two dots (model.py:802-810), lane 0 of them finishes the row
  const int ii = tid >> 3, t8 = tid & 7;
  const int64_t i = i0 + ii;
  const bool valid = i < b;
  const int64_t c = Lc[ii];
  float y = 0.f, tz = 0.f;
  for (int e = t8; e < D; e += 8) {
    y = fmaf(Lg[ii * pitch + e], p.H[c * D + e], y);
    tz = fmaf(p.U[user * D + e], p.Pp[c * D + e], tz);
  }
#pragma unroll
  for (int s = 1; s < 8; s <<= 1) {
    y += __shfl_xor(y, s);
    tz += __shfl_xor(tz, s);
  }
  float lterm = 0.f;
  if (t8 == 0) {
    float dl = 0.f;
    if (valid) {
      const float pr = sigmoidf(tz + y / float(h));
      const float lb = labels[i];
      // model.py:812: the log of an int64 tensor is taken in float32
      const float wt = 1.f + logf(float(1 + freq[i] * 10000000000ll));
      const float q = 1.f - pr;
      const float t1 = lb * logf(pr + 1e-10f), t2 = (1.f - lb) * logf(q + 1e-10f);
      lterm = -wt * (t1 + t2);
      // autograd's composed form: exactly 0 where p rounds to 0 or 1 (include/nais.h)
      const float gp = (-wt * lb) / (pr + 1e-10f) + (wt * (1.f - lb)) / (q + 1e-10f);
      dl = gp * q * pr;
      if (pred) pred[i] = pr;
      w.delta[i] = dl;
      w.dh[i] = dl / float(h);
      if (!(fabsf(lterm) <= 3.4028235e38f)) atomicAdd(bad_rows, 1);
    }
    Ld[ii] = dl;
  }
  // the wave's eight rows, then one atomic per wave
  lterm += __shfl_xor(lterm, 8);
  lterm += __shfl_xor(lterm, 16);
  lterm += __shfl_xor(lterm, 32);
  if (lane == 0) atomicAdd(loss_sum, lterm);
  __syncthreads();
  // this workgroup's part of dUserPreference[u] = sum_i delta_i PoiPreference[c_i]
  for (int e = tid; e < D; e += 256) {
    float g = 0.f;
#pragma unroll 8
    for (int r = 0; r < 32; ++r) g = fmaf(Ld[r], p.Pp[int64_t(Lc[r]) * D + e], g);
    w.upart[int64_t(blockIdx.x) * D + e] = g;
  }
}

// ---------------------------------------------------------------------------------------------
// dGeoInfluence: tile (32 e) x (32 j) of (diag(dh) Hs)^T . F, K = b over the eight waves
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * GT_KW) void geoie_step_geo_kernel(
    TP p, const int64_t* __restrict__ hist, uint32_t h, int64_t b, WS w, int ntj, float lr,
    float wd, const int32_t* __restrict__ err, float* __restrict__ g_out) {
  __shared__ float Lr[GT_KW * 1024];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 31, hh = lane >> 5;
  const int D = p.D;
  const int e0 = (int(blockIdx.x) / ntj) * 32;
  const uint32_t j0 = uint32_t(int(blockIdx.x) % ntj) * 32u;
  const int e = e0 + n;
  const uint32_t j = j0 + uint32_t(n);
  const bool eok = e < D, jok = j < h;
  const float* __restrict__ Hp = p.H;
  floatx16 C;
#pragma unroll
  for (int r = 0; r < 16; ++r) C[r] = 0.f;
#pragma unroll 4
  for (int64_t k0 = 2 * wave; k0 < b; k0 += 2 * GT_KW) {
    const int64_t k = k0 + hh;
    float av = 0.f, bv = 0.f;
    if (k < b) {   // the odd row past b is zero in both operands
      if (eok) av = w.dh[k] * Hp[int64_t(w.cidx[k]) * D + e];
      if (jok) bv = w.F[k * int64_t(h) + j];
    }
    C = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, C, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) Lr[wave * 1024 + r * 64 + lane] = C[r];
  __syncthreads();
  const bool apply = *err == 0;
  for (int o = tid; o < 1024; o += 64 * GT_KW) {
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < GT_KW; ++q) v += Lr[q * 1024 + o];
    const int r = o >> 6, ln = o & 63;
    const int ee = e0 + crow(r, ln >> 5);
    const uint32_t jj = j0 + uint32_t(ln & 31);
    if (ee < D && jj < h) {
      const uint32_t m = uint32_t(ee) * h + jj;      // flat position of Gr[ee][jj] (model.py:798)
      if (g_out) g_out[m] = v;
      if (apply) {
        const uint32_t rr = m / uint32_t(D);
        float* q = p.G + hist[rr] * D + (m - rr * uint32_t(D));
        *q = sgd_elem(*q, v, lr, wd);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// the target rows of PoiPreference / GeoSusceptibility and the user row
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void geoie_step_rows_kernel(
    TP p, int64_t user, int64_t b, int nblk, WS w, float lr, float wd,
    const int32_t* __restrict__ err, float* __restrict__ g_u, float* __restrict__ g_pp,
    float* __restrict__ g_h) {
  const int lane = threadIdx.x & 63, D = p.D;
  const int64_t item = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (item > b) return;
  const bool apply = *err == 0;
  if (item == b) {
    for (int e = lane; e < D; e += 64) {
      float g = 0.f;
      for (int q = 0; q < nblk; ++q) g += w.upart[int64_t(q) * D + e];
      if (g_u) g_u[e] = g;
      if (apply) p.U[user * D + e] = sgd_elem(w.uold[e], g, lr, wd);
    }
    return;
  }
  const int64_t c = w.cidx[item];
  const float dl = w.delta[item], dh = w.dh[item];
  for (int e = lane; e < D; e += 64) {
    const float gh = dh * w.T[item * D + e], gp = dl * w.uold[e];
    if (g_h) g_h[item * D + e] = gh;
    if (g_pp) g_pp[item * D + e] = gp;
    if (apply) {
      p.H[c * D + e] = sgd_elem(p.H[c * D + e], gh, lr, wd);
      p.Pp[c * D + e] = sgd_elem(p.Pp[c * D + e], gp, lr, wd);
    }
  }
}

// p -= lr * (g + weight_decay * p) over the rows whose stamp is not `tag` and that are not skip_row
__global__ __launch_bounds__(256) void sgd_rows_kernel(
    float* __restrict__ param, const float* __restrict__ grad, int64_t rows, int dim, float lr,
    float wd, const int32_t* __restrict__ stamp, int32_t tag, int64_t skip_row,
    const int32_t* __restrict__ err) {
  if (err && *err) return;
  const int64_t numel = rows * dim;
  for (int64_t x = int64_t(blockIdx.x) * 256 + threadIdx.x; x < numel; x += int64_t(gridDim.x) * 256) {
    const int64_t r = x / dim;
    if (r == skip_row || (stamp && stamp[r] == tag)) continue;
    param[x] = sgd_elem(param[x], grad ? grad[x] : 0.f, lr, wd);
  }
}

int check_params(const nais_geoie_params_t* q) {
  if (!q) return nais_internal_fail(NAIS_E_INVALID, "NULL params");
  if (q->embed_dim < 1 || q->embed_dim > 256)
    return nais_internal_fail(NAIS_E_UNSUPPORTED, "GeoIE embed_dim must be 1..256");
  if (q->num_pois < 1 || q->num_users < 1) return nais_internal_fail(NAIS_E_INVALID, "bad shape");
  if (q->num_pois >= (int64_t(1) << 24))
    return nais_internal_fail(NAIS_E_UNSUPPORTED, "GeoIE num_pois must be below 2^24");
  if (!q->user_pref || !q->poi_pref || !q->geo_influence || !q->geo_suscept)
    return nais_internal_fail(NAIS_E_INVALID, "NULL parameter pointer");
  return NAIS_OK;
}

int launch_sgd(float* param, const float* grad, int64_t rows, int dim, float lr, float wd,
               const int32_t* stamp, int32_t tag, int64_t skip_row, const int32_t* err,
               hipStream_t st) {
  const int64_t numel = rows * dim;
  const unsigned grid = unsigned(std::min<int64_t>((numel + 255) / 256, 4096));
  hipLaunchKernelGGL(sgd_rows_kernel, dim3(grid), dim3(256), 0, st, param, grad, rows, dim, lr, wd,
                     stamp, tag, skip_row, err);
  return nais_internal_check_launch("sgd_rows_kernel");
}

}  // namespace

extern "C" {

int32_t nais_geoie_make_train_batch(const int64_t* indptr, const int64_t* indices,
                                    const double* data, int64_t user, int64_t h, int64_t num_pois,
                                    int32_t num_ng, uint64_t seed, const double* coords,
                                    const double* dist_mat, int64_t* hist, int64_t* target,
                                    float* labels, int64_t* freq, float* distances, int64_t dist_ld,
                                    int32_t* err, void* stream) {
  if (!data || h < 1 || num_ng < 1 || dist_ld < h)
    return nais_internal_fail(NAIS_E_INVALID, "bad arguments (the history must not be empty)");
  if ((coords != nullptr) == (dist_mat != nullptr))
    return nais_internal_fail(NAIS_E_INVALID, "exactly one of coords and dist_mat");
  if (!freq || !distances) return nais_internal_fail(NAIS_E_INVALID, "NULL output");
  if (int rc = nais_make_train_batch(indptr, indices, user, h, num_pois, num_ng, seed, hist, target,
                                     labels, err, stream))
    return rc;
  const int64_t b = h * (1 + int64_t(num_ng));
  const int64_t nct = (h + 255) / 256, nrt = (b + GT_BR - 1) / GT_BR;
  if (nct * nrt > 0x7fffffffll) return nais_internal_fail(NAIS_E_UNSUPPORTED, "batch too large");
  hipLaunchKernelGGL(geoie_batch_fill_kernel, dim3((unsigned)(nct * nrt)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), indptr, data, user, h, b, (int)num_ng,
                     num_pois, coords, dist_mat, hist, target, freq, distances, dist_ld, nct);
  return nais_internal_check_launch("geoie_batch_fill_kernel");
}

size_t nais_geoie_train_step_workspace_size(const nais_geoie_params_t* params, int64_t b, int64_t h) {
  if (!params || b <= 0 || h <= 0) return 0;
  return ws_floats(b, h, params->embed_dim) * sizeof(float);
}

int32_t nais_geoie_train_step(const nais_geoie_params_t* params, int64_t user, const int64_t* hist,
                              int64_t h, const int64_t* target, const float* labels,
                              const int64_t* freq, int64_t b, const float* distances,
                              int64_t dist_ld, float lr, float weight_decay, int32_t* stamp_target,
                              int32_t* stamp_hist, int32_t tag, float* loss_sum, int32_t* bad_rows,
                              int32_t* err, float* pred, const nais_geoie_train_grads_t* grads,
                              void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_params(params)) return rc;
  const nais_geoie_params_t& q = *params;
  if (b < 1 || h < 1 || dist_ld < h || user < 0 || user >= q.num_users)
    return nais_internal_fail(NAIS_E_INVALID, "bad shape (the history must not be empty)");
  if (h >= (int64_t(1) << 22) || b >= (int64_t(1) << 26))
    return nais_internal_fail(NAIS_E_UNSUPPORTED, "batch too large");
  if (!hist || !target || !labels || !freq || !distances || !stamp_target || !stamp_hist ||
      !loss_sum || !bad_rows || !err)
    return nais_internal_fail(NAIS_E_INVALID, "NULL pointer");
  const int D = q.embed_dim;
  if (!workspace || workspace_bytes < ws_floats(b, h, D) * sizeof(float))
    return nais_internal_fail(NAIS_E_WORKSPACE, "workspace missing or too small");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  TP p{D, q.num_pois, const_cast<float*>(q.user_pref), const_cast<float*>(q.poi_pref),
       const_cast<float*>(q.geo_influence), const_cast<float*>(q.geo_suscept)};
  const WS w = carve(workspace, b, h, D);
  const int DP32 = (D + 31) & ~31, pitch = DP32 + 1;
  const int nblk = int((b + 31) / 32);
  const size_t lds = size_t(GT_JC * pitch + 32 * GT_FP + 64) * sizeof(float);
  static bool once = (hipFuncSetAttribute(reinterpret_cast<const void*>(geoie_step_fwd_kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024),
                      true);
  (void)once;
  hipLaunchKernelGGL(geoie_step_fwd_kernel, dim3((unsigned)nblk), dim3(256), lds, st, p, user, hist,
                     uint32_t(h), target, labels, freq, b, distances, dist_ld, q.a, q.b,
                     stamp_target, stamp_hist, tag, w, loss_sum, bad_rows, err, pred, pitch, DP32);
  if (int rc = nais_internal_check_launch("geoie_step_fwd_kernel")) return rc;
  const int ntj = int((h + 31) / 32);
  hipLaunchKernelGGL(geoie_step_geo_kernel, dim3((unsigned)((DP32 / 32) * ntj)), dim3(64 * GT_KW), 0,
                     st, p, hist, uint32_t(h), b, w, ntj, lr, weight_decay, err,
                     grads ? grads->geo_influence : nullptr);
  if (int rc = nais_internal_check_launch("geoie_step_geo_kernel")) return rc;
  hipLaunchKernelGGL(geoie_step_rows_kernel, dim3((unsigned)((b + 1 + 3) / 4)), dim3(256), 0, st, p,
                     user, b, nblk, w, lr, weight_decay, err, grads ? grads->user_pref : nullptr,
                     grads ? grads->poi_pref : nullptr, grads ? grads->geo_suscept : nullptr);
  if (int rc = nais_internal_check_launch("geoie_step_rows_kernel")) return rc;
  if (weight_decay != 0.f) {   // torch's dense SGD moves every element; the touched rows are done
    if (int rc = launch_sgd(p.U, nullptr, q.num_users, D, lr, weight_decay, nullptr, 0, user, err, st))
      return rc;
    if (int rc = launch_sgd(p.Pp, nullptr, q.num_pois, D, lr, weight_decay, stamp_target, tag, -1, err, st))
      return rc;
    if (int rc = launch_sgd(p.H, nullptr, q.num_pois, D, lr, weight_decay, stamp_target, tag, -1, err, st))
      return rc;
    if (int rc = launch_sgd(p.G, nullptr, q.num_pois, D, lr, weight_decay, stamp_hist, tag, -1, err, st))
      return rc;
  }
  return NAIS_OK;
}

int32_t nais_sgd(float* param, const float* grad, int64_t rows, int32_t dim, float lr,
                 float weight_decay, const int32_t* stamp, int32_t tag, int64_t skip_row,
                 const int32_t* err, void* stream) {
  if (rows < 0 || dim < 1) return nais_internal_fail(NAIS_E_INVALID, "bad shape");
  if (rows == 0) return NAIS_OK;
  if (!param) return nais_internal_fail(NAIS_E_INVALID, "NULL pointer");
  return launch_sgd(param, grad, rows, dim, lr, weight_decay, stamp, tag, skip_row, err,
                    reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
