// nais_geoie.hip -- the GeoIE model (model.py:757-828) on gfx950: the per-pair power-law table,
// the full-catalog scorer (validation.py:183-195 with get_GeoIE_batch_test, batches.py:244-269)
// and the batch forward. See include/nais.h "GeoIE" for the arithmetic.
//
// Scorer layout. One workgroup scores one user against 32 candidates per wave. The user's
// scrambled history Gr^T ([h, D]: Gr^T[j][e] = flat[e*h + j], model.py:798) is staged in LDS in
// chunks of GEOIE_JC rows, the wave's 32 GeoSusceptibility rows beside it, both at an odd pitch so
// that lanes over rows read distinct banks. One v_mfma_f32_32x32x2_f32 chain over e then forms
//   C (32 history entries x 32 candidates) = Gr^T_tile . H_tile^T      (exact fp32, k-ordered)
// and the epilogue folds C into y with the gathered table rows: lane (n, hh) holds candidate n and
// history rows crow(r, hh), so for a fixed r the 32 lanes of a half read 32 consecutive floats of
// one table row. The K extent is D rounded up to even; the padding column is zero in both
// operands and is added AFTER the scramble (the scramble indexes the unpadded h*D floats).
//
// Summation order (shared with the forward kernel, which therefore returns the same bits): S[j] is
// the fmaf chain over e = 0..D-1; y is two fmaf chains over ascending j, one per lane half
// (hh = (j >> 2) & 1, the 32x32 accumulator layout), added at the end; the preference dot is two
// fmaf chains over e = hh, hh + 2, ..., added at the end.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "nais_geo.h"
#include "nais_internal.h"

typedef float floatx16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int GEOIE_TR = 16;    // table rows per workgroup (their Geo staged once)
constexpr int GEOIE_JC = 64;    // history rows per LDS chunk of the scorer
constexpr int GEOIE_FJ = 256;   // history entries per pass of the forward kernel
constexpr int GEOIE_LDS_FLOATS = 160 * 1024 / 4;
static_assert(GEOIE_JC == 64, "the scorer's chunk staging takes a padded chunk to be 32 or 64 rows");

struct GP {
  int D;
  const float* U;
  const float* Pp;
  const float* G;
  const float* H;
};

// row of the 32x32 accumulator held in register r by lane half hh
__device__ __forceinline__ int crow(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

// min(max(0.01, d), 100) as Python evaluates it (run.py:44): max(0.01, nan) is 0.01
__device__ __forceinline__ double clamp_dist(double d) {
  const double lo = (d > 0.01) ? d : 0.01;
  return (100.0 < lo) ? 100.0 : lo;
}

__device__ __forceinline__ float sigmoidf(float s) { return 1.0f / (1.0f + expf(-s)); }

__global__ __launch_bounds__(256) void geoie_table_kernel(
    const double* __restrict__ coords, const double* __restrict__ dist_mat, int64_t P,
    const int64_t* __restrict__ items, int64_t J, int64_t col0, int64_t cols, int64_t nct, float a,
    float b, float* __restrict__ F, int64_t ld) {
  __shared__ Geo Lg[GEOIE_TR];
  __shared__ int64_t Li[GEOIE_TR];
  const int tid = threadIdx.x;
  const int64_t ct = int64_t(blockIdx.x) % nct, r0 = (int64_t(blockIdx.x) / nct) * GEOIE_TR;
  if (tid < GEOIE_TR && r0 + tid < J) {
    const int64_t it = items[r0 + tid];
    Li[tid] = it;
    if (coords) Lg[tid] = make_geo(coords[2 * it], coords[2 * it + 1]);
  }
  __syncthreads();
  const int64_t cc = ct * 256 + tid;
  if (cc >= cols) return;
  const int64_t c = col0 + cc;
  const int nr = (J - r0 < GEOIE_TR) ? int(J - r0) : GEOIE_TR;
  if (coords) {
    const Geo gc = make_geo(coords[2 * c], coords[2 * c + 1]);
    for (int i = 0; i < nr; ++i) {
      const double d = clamp_dist(ref_dist(gc, Lg[i]));   // dist(candidate, history), batches.py:256
      F[(r0 + i) * ld + cc] = a * powf(float(d), b);
    }
  } else {
    for (int i = 0; i < nr; ++i) F[(r0 + i) * ld + cc] = a * powf(float(dist_mat[c * P + Li[i]]), b);
  }
}

// rows [c0, c0 + 32) of a [P, D] table -> Lt [32][pitch], zero past `cend` and past column D
__device__ __forceinline__ void stage_tile(const float* __restrict__ tab, int D, int DP2, int pitch,
                                           int64_t c0, int64_t cend, float* Lt, int lane) {
#pragma unroll 4
  for (int idx = lane; idx < 32 * DP2; idx += 64) {
    const int rr = idx / DP2, k = idx - rr * DP2;
    Lt[rr * pitch + k] = (c0 + rr < cend && k < D) ? tab[(c0 + rr) * D + k] : 0.f;
  }
}

__global__ __launch_bounds__(256) void geoie_score_kernel(
    GP p, const int64_t* __restrict__ indptr, const int64_t* __restrict__ indices,
    const int32_t* __restrict__ users, int num_users, const int32_t* __restrict__ rowmap,
    const float* __restrict__ F, int64_t ld, int64_t J, int64_t col0, int64_t cols,
    float* __restrict__ scores, int64_t score_ld, int64_t score_col0, int32_t* __restrict__ nan_count,
    int pitch, int DP2) {
  extern __shared__ float geoie_lds[];
  const int tid = threadIdx.x, nt = blockDim.x, nw = nt >> 6, wave = tid >> 6, lane = tid & 63;
  const int n = lane & 31, hh = lane >> 5, D = p.D;
  float* Lg = geoie_lds;                                       // [GEOIE_JC][pitch]
  float* Lt = Lg + (GEOIE_JC + 32 * wave) * pitch;             // [32][pitch], this wave's
  float* Lu = geoie_lds + (GEOIE_JC + 32 * nw) * pitch;        // [DP2]
  int* Lrow = reinterpret_cast<int*>(Lu + DP2);                // [GEOIE_JC]
  const int slot = int(blockIdx.x % unsigned(num_users));
  const int64_t tile = blockIdx.x / unsigned(num_users);
  const int64_t u = users[slot];
  const int64_t beg = indptr[u];
  const uint32_t h = uint32_t(indptr[u + 1] - beg);
  const int64_t* __restrict__ hist = indices + beg;
  const float* __restrict__ Gp = p.G;
  const int64_t cbase = tile * (32 * nw) + 32 * wave;          // wave-uniform
  const bool wave_on = cbase < cols;
  const int64_t cc = cbase + n;
  const bool valid = cc < cols;
  const int64_t c = col0 + cc;

  // preference dot UserPreference[u] . PoiPreference[c] (model.py:805-808)
  for (int k = tid; k < DP2; k += nt) Lu[k] = (k < D) ? p.U[u * D + k] : 0.f;
  stage_tile(p.Pp, D, DP2, pitch, col0 + cbase, col0 + cols, Lt, lane);
  __syncthreads();
  float t = 0.f;
  for (int k = hh; k < DP2; k += 2) t = fmaf(Lu[k], Lt[n * pitch + k], t);
  const float tz = t + __shfl_xor(t, 32);
  __syncthreads();
  stage_tile(p.H, D, DP2, pitch, col0 + cbase, col0 + cols, Lt, lane);

  float y = 0.f;
  for (uint32_t jc0 = 0; jc0 < h; jc0 += GEOIE_JC) {
    __syncthreads();   // the previous chunk is consumed (first pass: the H tiles are staged)
    const int nj = (h - jc0 < uint32_t(GEOIE_JC)) ? int(h - jc0) : GEOIE_JC;
    const int njp = (nj + 31) & ~31;
    // Gr^T rows [jc0, jc0 + nj): consecutive threads take consecutive j, i.e. consecutive
    // elements m = e*h + j of the flat gather (coalesced within an embedding row)
    const int sh = (njp == 32) ? 5 : 6;   // njp is 32 or 64
#pragma unroll 4
    for (int idx = tid; idx < njp * DP2; idx += nt) {
      const int e = idx >> sh, jj = idx & (njp - 1);
      float v = 0.f;
      if (jj < nj && e < D) {
        const uint32_t m = uint32_t(e) * h + jc0 + uint32_t(jj);
        const uint32_t r = m / uint32_t(D);
        v = Gp[hist[r] * D + (m - r * uint32_t(D))];
      }
      Lg[jj * pitch + e] = v;
    }
    for (int jj = tid; jj < nj; jj += nt) Lrow[jj] = rowmap[hist[jc0 + jj]];
    __syncthreads();
    if (wave_on) {
      for (int jt = 0; jt < njp; jt += 32) {
        // the 16 table values of this lane's accumulator rows, requested before the MFMA chain so
        // that their latency runs under it. Every load is unconditional: a lane or row that does
        // not count reads F[0] (num_items >= 1, cols >= 1) and its value is dropped below
        float fv[16];
        bool ok[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int jl = jt + crow(r, hh);
          const int64_t fr = (jl < nj) ? Lrow[jl] : -1;
          ok[r] = valid && fr >= 0 && fr < J;
          fv[r] = F[ok[r] ? fr * ld + cc : 0];
        }
        floatx16 C;
#pragma unroll
        for (int r = 0; r < 16; ++r) C[r] = 0.f;
        const float* ap = Lg + (jt + n) * pitch + hh;
        const float* bp = Lt + n * pitch + hh;
        for (int k0 = 0; k0 < DP2; k0 += 2)
          C = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[k0], bp[k0], C, 0, 0, 0);
        // selects and fmafs only: no cross-lane reads under a per-lane condition
#pragma unroll
        for (int r = 0; r < 16; ++r) y = ok[r] ? fmaf(C[r], fv[r], y) : y;
      }
    }
  }
  const float yt = y + __shfl_xor(y, 32);
  const float sc = sigmoidf(tz + yt / float(h));
  if (valid && hh == 0) {
    // history POIs are not candidates (batches.py:250); the CSR row is ascending
    uint32_t lo = 0, hi = h;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (hist[mid] < c) lo = mid + 1; else hi = mid;
    }
    const bool in_hist = lo < h && hist[lo] == c;
    scores[int64_t(slot) * score_ld + (c - score_col0)] = in_hist ? -1.0f : sc;
    if (nan_count && !in_hist && sc != sc) atomicAdd(nan_count, 1);
  }
}

__global__ __launch_bounds__(64) void geoie_forward_kernel(
    GP p, const int64_t* __restrict__ user, const int64_t* __restrict__ target,
    const int64_t* __restrict__ hist, uint32_t n, int64_t hist_ld, const float* __restrict__ dist,
    int64_t dist_ld, float a, float b, float* __restrict__ out) {
  __shared__ float Ls[GEOIE_FJ], Lf[GEOIE_FJ];
  const int lane = threadIdx.x, D = p.D;
  const int64_t i = blockIdx.x;
  const int64_t u = user[i], c = target[i];
  const int64_t* hrow = hist + i * hist_ld;
  const float* drow = dist + i * dist_ld;
  float y = 0.f;
  for (uint32_t j0 = 0; j0 < n; j0 += GEOIE_FJ) {
    const int cnt = (n - j0 < uint32_t(GEOIE_FJ)) ? int(n - j0) : GEOIE_FJ;
    for (int jj = lane; jj < cnt; jj += 64) {
      const uint32_t j = j0 + uint32_t(jj);
      float S = 0.f;
      for (int e = 0; e < D; ++e) {
        const uint32_t m = uint32_t(e) * n + j;
        const uint32_t r = m / uint32_t(D);
        S = fmaf(p.G[hrow[r] * D + (m - r * uint32_t(D))], p.H[c * D + e], S);
      }
      Ls[jj] = S;
      Lf[jj] = a * powf(drow[j], b);
    }
    __syncthreads();
    if (lane < 2)   // the scorer's two lane halves: hh = (j >> 2) & 1 (GEOIE_FJ is a multiple of 8)
      for (int jj = 0; jj < cnt; ++jj)
        if (((jj >> 2) & 1) == lane) y = fmaf(Ls[jj], Lf[jj], y);
    __syncthreads();
  }
  float t = 0.f;
  if (lane < 2)
    for (int k = lane; k < D; k += 2) t = fmaf(p.U[u * D + k], p.Pp[c * D + k], t);
  const float yt = y + __shfl_xor(y, 1);
  const float tz = t + __shfl_xor(t, 1);
  if (lane == 0) out[i] = sigmoidf(tz + yt / float(n));
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

}  // namespace

extern "C" {

int32_t nais_geoie_table(const double* coords, const double* dist_mat, int64_t num_pois,
                         const int64_t* items, int64_t num_items, int64_t col0, int64_t cols,
                         float a, float b, float* f, int64_t ld, void* stream) {
  if (num_pois < 1 || num_items < 0 || cols < 0 || col0 < 0 || col0 + cols > num_pois || ld < cols)
    return nais_internal_fail(NAIS_E_INVALID, "bad shape");
  if ((coords != nullptr) == (dist_mat != nullptr))
    return nais_internal_fail(NAIS_E_INVALID, "exactly one of coords and dist_mat");
  if (num_items == 0 || cols == 0) return NAIS_OK;
  if (!items || !f) return nais_internal_fail(NAIS_E_INVALID, "NULL pointer");
  const int64_t nct = (cols + 255) / 256, nrt = (num_items + GEOIE_TR - 1) / GEOIE_TR;
  if (nct * nrt > 0x7fffffffll) return nais_internal_fail(NAIS_E_UNSUPPORTED, "table too large");
  hipLaunchKernelGGL(geoie_table_kernel, dim3((unsigned)(nct * nrt)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), coords, dist_mat, num_pois, items,
                     num_items, col0, cols, nct, a, b, f, ld);
  return nais_internal_check_launch("geoie_table_kernel");
}

int32_t nais_geoie_score(const nais_geoie_params_t* params, const int64_t* indptr,
                         const int64_t* indices, const int32_t* users, int32_t num_users,
                         const int32_t* rowmap, const float* f, int64_t ld, int64_t num_items,
                         int64_t col0, int64_t cols, float* scores, int64_t score_ld,
                         int64_t score_col0, int32_t* nan_count, void* stream) {
  if (int rc = check_params(params)) return rc;
  const nais_geoie_params_t& q = *params;
  if (num_users < 0 || cols < 0 || col0 < 0 || col0 + cols > q.num_pois || ld < cols ||
      num_items < 1 || score_col0 < 0 || score_col0 > col0 ||
      score_ld < col0 + cols - score_col0)
    return nais_internal_fail(NAIS_E_INVALID, "bad shape");
  if (num_users == 0 || cols == 0) return NAIS_OK;
  if (!indptr || !indices || !users || !rowmap || !f || !scores)
    return nais_internal_fail(NAIS_E_INVALID, "NULL pointer");
  const int D = q.embed_dim, DP2 = (D + 1) & ~1, pitch = DP2 + 1;
  // four waves (128 candidates) per workgroup where their tiles fit the LDS beside the history
  // chunk, else two (embed_dim above ~180)
  int nw = 4;
  auto floats = [&](int w) { return (GEOIE_JC + 32 * w) * pitch + DP2 + GEOIE_JC; };
  if (floats(nw) > GEOIE_LDS_FLOATS) nw = 2;
  const int64_t ntiles = (cols + 32 * nw - 1) / (32 * nw);
  if (ntiles * num_users > 0x7fffffffll) return nais_internal_fail(NAIS_E_UNSUPPORTED, "job too large");
  static bool once = (hipFuncSetAttribute(reinterpret_cast<const void*>(geoie_score_kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024),
                      true);
  (void)once;
  GP p{D, q.user_pref, q.poi_pref, q.geo_influence, q.geo_suscept};
  hipLaunchKernelGGL(geoie_score_kernel, dim3((unsigned)(ntiles * num_users)), dim3(64 * nw),
                     size_t(floats(nw)) * 4, reinterpret_cast<hipStream_t>(stream), p, indptr, indices,
                     users, num_users, rowmap, f, ld, num_items, col0, cols, scores, score_ld,
                     score_col0, nan_count, pitch, DP2);
  return nais_internal_check_launch("geoie_score_kernel");
}

int32_t nais_geoie_forward(const nais_geoie_params_t* params, const int64_t* user,
                           const int64_t* target, const int64_t* hist, int64_t b, int64_t n,
                           int64_t hist_ld, const float* distances, int64_t dist_ld, float* out,
                           void* stream) {
  if (int rc = check_params(params)) return rc;
  const nais_geoie_params_t& q = *params;
  if (b < 0 || n < 1 || hist_ld < n || dist_ld < n)
    return nais_internal_fail(NAIS_E_INVALID, "bad shape (the history must not be empty)");
  if (n >= (int64_t(1) << 24)) return nais_internal_fail(NAIS_E_UNSUPPORTED, "history too long");
  if (b == 0) return NAIS_OK;
  if (b > 0x7fffffffll) return nais_internal_fail(NAIS_E_UNSUPPORTED, "b too large");
  if (!user || !target || !hist || !distances || !out)
    return nais_internal_fail(NAIS_E_INVALID, "NULL pointer");
  GP p{q.embed_dim, q.user_pref, q.poi_pref, q.geo_influence, q.geo_suscept};
  hipLaunchKernelGGL(geoie_forward_kernel, dim3((unsigned)b), dim3(64), 0,
                     reinterpret_cast<hipStream_t>(stream), p, user, target, hist, uint32_t(n), hist_ld,
                     distances, dist_ld, q.a, q.b, out);
  return nais_internal_check_launch("geoie_forward_kernel");
}

}  // extern "C"
