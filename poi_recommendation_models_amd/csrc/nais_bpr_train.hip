// nais_bpr_train.hip -- BPR training on gfx950: the device-side get_BPR_batch (batches.py:6-22)
// and the fused step forward + loss + backward + SGD (run.py:504-509). See include/nais.h
// "BPR training" for the arithmetic.
//
// A batch is n triples (u, i, j) in which users and items repeat; every repeat is summed before
// the one SGD update of its row, and the sums must not depend on scheduling. So there is no
// float atomic on a table: the caller passes a stable sort of the n user ids and of the 2n item
// ids (item_i then item_j), and one wave per sorted position that starts a run of equal ids walks
// the run in order, lanes over the embedding dims.
//
//   bpr_step_fwd_kernel    one thread per triple: the two dots (the forward kernel's fmaf chain),
//                          s, the loss term and g; the stamps; ids checked. The loss terms are
//                          summed per workgroup in a fixed tree.
//   bpr_step_users_kernel  runs of the user order: dU[u] = sum g (I[i] - I[j]) from the pre-step
//                          item table; the updated row goes to a staging buffer.
//   bpr_step_items_kernel  runs of the item order: dI[c] = sum +-g U[u] from the pre-step user
//                          table (still untouched), updated in place -- the user kernel has
//                          finished reading the item table.
//   bpr_step_commit_kernel the staged user rows into the table; the loss partials, in order,
//                          into *loss_sum.
//   nais_sgd               weight_decay != 0 only: the rows the step did not touch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "nais_bpr_common.h"
#include "nais_internal.h"
#include "nais_sampler.h"

namespace {

constexpr int BT_ROWS = 4;      // runs (waves) per workgroup of the row kernels
constexpr int BT_MAXD = 256;

struct TB {
  int D;
  int64_t U, P;
  float* eu;
  float* ei;
};

struct WS {
  float* g;         // [n]
  float* part;      // [ceil(n / 256)] loss partials
  float* newu;      // [n, D] updated user rows, at the sorted position that starts the run
};

size_t ws_floats(int64_t n, int64_t D) { return size_t(n + (n + 255) / 256 + n * D + 16); }

WS carve(void* w, int64_t n) {
  WS s;
  s.g = static_cast<float*>(w);
  s.part = s.g + n;
  s.newu = s.part + (n + 255) / 256;
  return s;
}

// torch.optim.SGD without momentum: g' = g + weight_decay * p; p -= lr * g'
__device__ __forceinline__ float sgd_elem(float p, float g, float lr, float wd) {
  const float gg = (wd != 0.f) ? fmaf(wd, p, g) : g;
  return fmaf(-lr, gg, p);
}

__device__ __forceinline__ float chain_dot(const float* __restrict__ a,
                                           const float* __restrict__ b, int D) {
  float s = 0.f;
  for (int e = 0; e < D; ++e) s = fmaf(a[e], b[e], s);
  return s;
}

__global__ __launch_bounds__(256) void bpr_step_fwd_kernel(
    TB p, const int64_t* __restrict__ user, const int64_t* __restrict__ item_i,
    const int64_t* __restrict__ item_j, int64_t n, int32_t* __restrict__ st_u,
    int32_t* __restrict__ st_i, int32_t tag, WS w, int32_t* __restrict__ err,
    float* __restrict__ pred_i, float* __restrict__ pred_j, float* __restrict__ g_out) {
  __shared__ float Ll[256];
  const int tid = threadIdx.x;
  const int64_t t = int64_t(blockIdx.x) * 256 + tid;
  float lterm = 0.f;
  if (t < n) {
    const int64_t u = user[t], i = item_i[t], j = item_j[t];
    float g = 0.f;
    if (u < 0 || u >= p.U || i < 0 || i >= p.P || j < 0 || j >= p.P) {
      atomicOr(err, 2);
    } else {
      const float xi = chain_dot(p.eu + u * p.D, p.ei + i * p.D, p.D);
      const float xj = chain_dot(p.eu + u * p.D, p.ei + j * p.D, p.D);
      const float s = 1.0f / (1.0f + expf(-(xi - xj)));
      lterm = -logf(s);
      // autograd's composed form (log, then sigmoid): NaN where s rounds to 0 (include/nais.h)
      g = (-1.0f / s) * ((1.0f - s) * s);
      st_u[u] = tag;
      st_i[i] = tag;
      st_i[j] = tag;
      if (pred_i) pred_i[t] = xi;
      if (pred_j) pred_j[t] = xj;
    }
    w.g[t] = g;
    if (g_out) g_out[t] = g;
  }
  Ll[tid] = lterm;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) Ll[tid] += Ll[tid + s];
    __syncthreads();
  }
  if (tid == 0) w.part[blockIdx.x] = Ll[0];
}

// one wave per sorted position q; the wave whose position starts a run of equal user ids sums it
__global__ __launch_bounds__(64 * BT_ROWS) void bpr_step_users_kernel(
    TB p, const int64_t* __restrict__ user, const int64_t* __restrict__ item_i,
    const int64_t* __restrict__ item_j, int64_t n, const int64_t* __restrict__ order, WS w,
    float lr, float wd, const int32_t* __restrict__ err, float* __restrict__ g_u) {
  const int lane = threadIdx.x & 63, D = p.D;
  const int64_t q = int64_t(blockIdx.x) * BT_ROWS + (threadIdx.x >> 6);
  if (q >= n || *err) return;
  auto at = [&](int64_t qq) -> int64_t {
    const int64_t t = order ? order[qq] : qq;
    return (t < 0 || t >= n) ? -1 : t;
  };
  const int64_t t0 = at(q);
  if (t0 < 0) return;   // not a permutation: reported by the forward kernel's caller contract
  const int64_t u = user[t0];
  if (q > 0) {
    const int64_t tp = at(q - 1);
    if (tp >= 0 && user[tp] == u) return;
  }
  float acc[BT_MAXD / 64];
#pragma unroll
  for (int x = 0; x < BT_MAXD / 64; ++x) acc[x] = 0.f;
  for (int64_t qq = q; qq < n; ++qq) {
    const int64_t t = at(qq);
    if (t < 0 || user[t] != u) break;
    const float g = w.g[t];
    const float* __restrict__ ri = p.ei + item_i[t] * D;
    const float* __restrict__ rj = p.ei + item_j[t] * D;
#pragma unroll
    for (int x = 0; x < BT_MAXD / 64; ++x) {
      const int e = lane + 64 * x;
      if (e < D) acc[x] = fmaf(g, ri[e] - rj[e], acc[x]);
    }
  }
#pragma unroll
  for (int x = 0; x < BT_MAXD / 64; ++x) {
    const int e = lane + 64 * x;
    if (e < D) {
      if (g_u) g_u[u * D + e] = acc[x];
      w.newu[q * D + e] = sgd_elem(p.eu[u * D + e], acc[x], lr, wd);
    }
  }
}

// the same over the 2n item keys: sorted entry x < n is item_i[x] (+g), else item_j[x - n] (-g)
__global__ __launch_bounds__(64 * BT_ROWS) void bpr_step_items_kernel(
    TB p, const int64_t* __restrict__ user, const int64_t* __restrict__ item_i,
    const int64_t* __restrict__ item_j, int64_t n, const int64_t* __restrict__ order, WS w,
    float lr, float wd, const int32_t* __restrict__ err, float* __restrict__ g_i) {
  const int lane = threadIdx.x & 63, D = p.D;
  const int64_t q = int64_t(blockIdx.x) * BT_ROWS + (threadIdx.x >> 6);
  if (q >= 2 * n || *err) return;
  auto key = [&](int64_t qq, int64_t* t, float* sign) -> int64_t {
    const int64_t x = order[qq];
    if (x < 0 || x >= 2 * n) return -1;
    *t = (x < n) ? x : x - n;
    *sign = (x < n) ? 1.f : -1.f;
    return (x < n) ? item_i[*t] : item_j[*t];
  };
  int64_t t;
  float sign;
  const int64_t c = key(q, &t, &sign);
  if (c < 0) return;
  if (q > 0 && key(q - 1, &t, &sign) == c) return;
  float acc[BT_MAXD / 64];
#pragma unroll
  for (int x = 0; x < BT_MAXD / 64; ++x) acc[x] = 0.f;
  for (int64_t qq = q; qq < 2 * n; ++qq) {
    if (key(qq, &t, &sign) != c) break;
    const float g = sign * w.g[t];
    const float* __restrict__ ru = p.eu + user[t] * D;
#pragma unroll
    for (int x = 0; x < BT_MAXD / 64; ++x) {
      const int e = lane + 64 * x;
      if (e < D) acc[x] = fmaf(g, ru[e], acc[x]);
    }
  }
#pragma unroll
  for (int x = 0; x < BT_MAXD / 64; ++x) {
    const int e = lane + 64 * x;
    if (e < D) {
      if (g_i) g_i[c * D + e] = acc[x];
      p.ei[c * D + e] = sgd_elem(p.ei[c * D + e], acc[x], lr, wd);
    }
  }
}

__global__ __launch_bounds__(64 * BT_ROWS) void bpr_step_commit_kernel(
    TB p, const int64_t* __restrict__ user, int64_t n, const int64_t* __restrict__ order, WS w,
    int64_t nparts, const int32_t* __restrict__ err, float* __restrict__ loss_sum) {
  const int lane = threadIdx.x & 63, D = p.D;
  const int64_t q = int64_t(blockIdx.x) * BT_ROWS + (threadIdx.x >> 6);
  if (q == 0 && lane == 0) {   // the loss is reported even when the step is not applied
    float l = 0.f;
    for (int64_t b = 0; b < nparts; ++b) l += w.part[b];
    *loss_sum += l;
  }
  if (q >= n || *err) return;
  auto at = [&](int64_t qq) -> int64_t {
    const int64_t t = order ? order[qq] : qq;
    return (t < 0 || t >= n) ? -1 : t;
  };
  const int64_t t0 = at(q);
  if (t0 < 0) return;
  const int64_t u = user[t0];
  if (q > 0) {
    const int64_t tp = at(q - 1);
    if (tp >= 0 && user[tp] == u) return;
  }
  for (int e = lane; e < D; e += 64) p.eu[u * D + e] = w.newu[q * D + e];
}

// ---------------------------------------------------------------------------------------------
// get_BPR_batch (batches.py:6-22): one workgroup per listed user
// ---------------------------------------------------------------------------------------------
constexpr int BB_THREADS = 256;

__global__ __launch_bounds__(BB_THREADS) void bpr_make_batch_kernel(
    const int64_t* __restrict__ indptr, const int64_t* __restrict__ indices, int64_t num_rows,
    const int64_t* __restrict__ users, const int64_t* __restrict__ offsets, int64_t P, uint32_t s1,
    int64_t* __restrict__ out_u, int64_t* __restrict__ out_i, int64_t* __restrict__ out_j,
    int32_t* __restrict__ err) {
  __shared__ int32_t scan[BB_THREADS / 64];
  __shared__ int64_t base;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t u = users[blockIdx.x];
  if (u < 0 || u >= num_rows) {
    if (tid == 0) atomicOr(err, 2);
    return;
  }
  const int64_t start = indptr[u], h = indptr[u + 1] - start, off = offsets[blockIdx.x];
  if (h > P - h) {   // the reference's negative[i] raises (batches.py:14-16)
    if (tid == 0) atomicOr(err, 1);
    return;
  }
  const int64_t* row = indices + start;
  for (int64_t i = tid; i < h; i += BB_THREADS) {
    out_u[off + i] = u;
    out_i[off + i] = row[i];
  }
  // the first h members, in a seeded pseudo-random order of [0, P), that are not positives
  // (nais_make_train_batch's sampler, one seed per user): among the first 2h at most h are
  const uint32_t mP = uint32_t(P), su = mix32(s1 ^ mix32(uint32_t(u) + 0x9e3779b9u));
  const int hP = mP > 1 ? half_bits(mP) : 0;
  if (tid == 0) base = 0;
  __syncthreads();
  for (int64_t k0 = 0; k0 < 2 * h; k0 += BB_THREADS) {
    const int64_t k = k0 + tid;
    int64_t cand = -1;
    if (k < 2 * h) {
      cand = mP > 1 ? permute(uint32_t(k), mP, hP, su) : 0;
      int64_t lo = 0, hi = h;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (row[mid] < cand) lo = mid + 1;
        else hi = mid;
      }
      if (lo < h && row[lo] == cand) cand = -1;
    }
    const bool acc = cand >= 0;
    const unsigned long long bal = __ballot(acc);
    const int before = __popcll(bal & ((1ull << lane) - 1));
    if (lane == 0) scan[w] = __popcll(bal);
    __syncthreads();
    int o = 0, tot = 0;
    for (int q = 0; q < BB_THREADS / 64; ++q) {
      if (q < w) o += scan[q];
      tot += scan[q];
    }
    const int64_t pos = base + o + before;
    if (acc && pos < h) out_j[off + pos] = cand;
    __syncthreads();
    if (tid == 0) base += tot;
    __syncthreads();
  }
}

}  // namespace

extern "C" {

int32_t nais_bpr_make_train_batch(const int64_t* indptr, const int64_t* indices,
                                  int64_t num_rows, const int64_t* users, const int64_t* offsets, int64_t num_users,
                                  int64_t num_pois, uint64_t seed, int64_t* user, int64_t* item_i,
                                  int64_t* item_j, int32_t* err, void* stream) {
  if (!indptr || num_rows < 1 || num_users < 0 || num_pois <= 0)   // indices may be NULL: a CSR without entries
    return nais_internal_fail(NAIS_E_INVALID, "bad arguments");
  if (num_pois > 0x7fffffffll || num_users > 0x7fffffffll)
    return nais_internal_fail(NAIS_E_UNSUPPORTED, "num_pois / num_users must fit 31 bits");
  if (num_users == 0) return NAIS_OK;
  if (!users || !offsets || !user || !item_i || !item_j || !err)
    return nais_internal_fail(NAIS_E_INVALID, "NULL pointer");
  hipLaunchKernelGGL(bpr_make_batch_kernel, dim3((unsigned)num_users), dim3(BB_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), indptr, indices, num_rows, users,
                     offsets, num_pois, mix32(uint32_t(seed >> 32) ^ uint32_t(seed) * 0x9e3779b9u), user,
                     item_i, item_j, err);
  return nais_internal_check_launch("bpr_make_batch_kernel");
}

size_t nais_bpr_train_step_workspace_size(const nais_bpr_params_t* params, int64_t n) {
  if (!params || n <= 0) return 0;
  return ws_floats(n, params->embed_dim) * sizeof(float);
}

int32_t nais_bpr_train_step(const nais_bpr_params_t* params, const int64_t* user,
                            const int64_t* item_i, const int64_t* item_j, int64_t n,
                            const int64_t* user_order, const int64_t* item_order, float lr,
                            float weight_decay, int32_t* stamp_user, int32_t* stamp_item,
                            int32_t tag, float* loss_sum, int32_t* err, float* pred_i,
                            float* pred_j, float* g, const nais_bpr_train_grads_t* grads,
                            void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = nais_bpr_check_params(params)) return rc;
  const nais_bpr_params_t& q = *params;
  if (n < 1) return nais_internal_fail(NAIS_E_INVALID, "bad shape (n must be at least 1)");
  if (n >= (int64_t(1) << 28)) return nais_internal_fail(NAIS_E_UNSUPPORTED, "batch too large");
  if (!user || !item_i || !item_j || !item_order || !stamp_user || !stamp_item || !loss_sum || !err)
    return nais_internal_fail(NAIS_E_INVALID, "NULL pointer");
  const int D = q.embed_dim;
  if (!workspace || workspace_bytes < ws_floats(n, D) * sizeof(float))
    return nais_internal_fail(NAIS_E_WORKSPACE, "workspace missing or too small");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  TB p{D, q.num_users, q.num_pois, const_cast<float*>(q.embed_user), const_cast<float*>(q.embed_item)};
  const WS w = carve(workspace, n);
  const int64_t nparts = (n + 255) / 256;
  hipLaunchKernelGGL(bpr_step_fwd_kernel, dim3((unsigned)nparts), dim3(256), 0, st, p, user, item_i,
                     item_j, n, stamp_user, stamp_item, tag, w, err, pred_i, pred_j, g);
  if (int rc = nais_internal_check_launch("bpr_step_fwd_kernel")) return rc;
  const unsigned gu = unsigned((n + BT_ROWS - 1) / BT_ROWS), gi = unsigned((2 * n + BT_ROWS - 1) / BT_ROWS);
  hipLaunchKernelGGL(bpr_step_users_kernel, dim3(gu), dim3(64 * BT_ROWS), 0, st, p, user, item_i,
                     item_j, n, user_order, w, lr, weight_decay, err,
                     grads ? grads->embed_user : nullptr);
  if (int rc = nais_internal_check_launch("bpr_step_users_kernel")) return rc;
  hipLaunchKernelGGL(bpr_step_items_kernel, dim3(gi), dim3(64 * BT_ROWS), 0, st, p, user, item_i,
                     item_j, n, item_order, w, lr, weight_decay, err,
                     grads ? grads->embed_item : nullptr);
  if (int rc = nais_internal_check_launch("bpr_step_items_kernel")) return rc;
  hipLaunchKernelGGL(bpr_step_commit_kernel, dim3(gu), dim3(64 * BT_ROWS), 0, st, p, user, n,
                     user_order, w, nparts, err, loss_sum);
  if (int rc = nais_internal_check_launch("bpr_step_commit_kernel")) return rc;
  if (weight_decay != 0.f) {   // torch's dense SGD moves every element; the touched rows are done
    if (int rc = nais_sgd(p.eu, nullptr, q.num_users, D, lr, weight_decay, stamp_user, tag, -1, err, stream))
      return rc;
    if (int rc = nais_sgd(p.ei, nullptr, q.num_pois, D, lr, weight_decay, stamp_item, tag, -1, err, stream))
      return rc;
  }
  return NAIS_OK;
}

}  // extern "C"
