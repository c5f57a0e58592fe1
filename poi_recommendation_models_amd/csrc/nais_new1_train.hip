// nais_new1_train.hip -- New1 training on gfx950: the device-side trainDataset.__getitem__
// (run_new.py:107-137) and the fused step forward + BCELoss + backward + torch.optim.Adam
// (run_new.py:403-410, model.py:861-918). See include/nais.h "New1 training" for the arithmetic
// and DESIGN.md "New1 training" for the split.
//
// One batch is one user: b target rows that all share ONE history hist[n]. With T, Q the target
// rows' concatenated embeddings and attn_Q projections, H, K, V the same for the history and
// Ks = the contiguous [n, d] key buffer READ AS a row-major [d, n] matrix (model.py:896), every
// product of the step is a small dense GEMM  C[m][c] = sum_k A(k, m) B(k, c)  between buffers of
// the workspace. They all run through ONE kernel, new1_gemm_kernel: a workgroup of eight waves per
// 32 x 32 tile of C, the K extent dealt to the waves in pairs (v_mfma_f32_32x32x2_f32, exact
// fp32), the eight partial tiles summed in LDS in wave order. A launch carries a list of jobs
// (tiles of several products that do not depend on each other), so a step is eight launches:
//
//   new1_rows_gather_kernel  H [n, d], T [b, d] gathered into the workspace, one wave per row; ids
//                            checked (range, repeats through the [P] stamps), the rows' slots
//                            recorded, g = sum_j r_j h_j by one more workgroup.
//   gemm  1                  K = H Wk^T, V = H Wv^T, Q = T Wq^T
//   gemm  2                  A = Q Ks,  M = T V^T                                  ([b, n] each)
//   new1_rows_loss_kernel    one wave per target row: E, S, N, pred, x, the loss term, delta, and
//                            dA / sqrt(d), dM written over A, M
//   gemm  3                  dQ = dA Ks^T, dTv = dM V, dKs = Q^T dA, dV = dM^T T, dg = delta^T T
//   gemm  4                  dT = dQ Wq + dTv + delta g^T,  dH = dK Wk + dV Wv + r dg^T,
//                            dWq = dQ^T T, dWk = dK^T H, dWv = dV^T H
//   new1_adam_dense_kernel   embed_target (every row; a touched row finds its dT / dH rows through
//                            the slot maps) and the three d x d weights
//   new1_adam_region_kernel  one wave per embed_region row: the ordered segment sum of the dT / dH
//                            right halves of the rows of that region (targets in batch order, then
//                            the history), then Adam; one more wave sums the loss terms in order.
//
// Nothing is added with float atomics: the same batch from the same state gives the same bits.
// Ids outside their tables, repeated targets or history entries and a NaN prediction set *err;
// both Adam kernels write nothing while *err is set.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "nais_internal.h"
#include "nais_sampler.h"

typedef float floatx16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int NT_KW = 8;          // waves of the GEMM kernel (they split K)
constexpr int NT_MAXJOBS = 5;     // products per GEMM launch
constexpr int NT_BATCH_THREADS = 1024;

__device__ __forceinline__ int crow(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

struct NP1T {
  int d;
  int64_t P, R;
  float beta;
  float *E, *Er, *Wq, *Wk, *Wv;
};

// workspace carve-up, shared by every kernel of the step
struct WS {
  float *H, *T, *Q, *K, *V;       // [n, d], [b, d], [b, d], [n, d], [n, d]
  float *A, *M;                   // [b, n] each: logits -> E -> dA / sqrt(d);  T.V -> dM
  float *dQ, *dTv, *dT;           // [b, d]
  float *dK, *dV, *dH;            // [n, d]   (dK is dKs [d, n] read back as [n, d])
  float *dWq, *dWk, *dWv;         // [d, d]
  float *g, *dg;                  // [d]
  float *delta, *lterm;           // [b]
  int32_t *treg, *hreg;           // [b], [n]  region ids, -1 outside the table
  int32_t *slot_t, *slot_h;       // [P]  row of T / H that holds POI p, valid where stamp == tag
};

size_t ws_bytes(int64_t b, int64_t n, int64_t d, int64_t P) {
  const int64_t fl = 5 * b * d + 6 * n * d + 2 * b * n + 3 * d * d + 2 * d + 2 * b;
  return size_t(fl + b + n + 2 * P + 64) * 4;
}

WS carve(void* w, int64_t b, int64_t n, int64_t d, int64_t P) {
  WS s;
  float* f = static_cast<float*>(w);
  s.H = f;            f += n * d;
  s.T = f;            f += b * d;
  s.Q = f;            f += b * d;
  s.K = f;            f += n * d;
  s.V = f;            f += n * d;
  s.A = f;            f += b * n;
  s.M = f;            f += b * n;
  s.dQ = f;           f += b * d;
  s.dTv = f;          f += b * d;
  s.dT = f;           f += b * d;
  s.dK = f;           f += n * d;
  s.dV = f;           f += n * d;
  s.dH = f;           f += n * d;
  s.dWq = f;          f += d * d;
  s.dWk = f;          f += d * d;
  s.dWv = f;          f += d * d;
  s.g = f;            f += d;
  s.dg = f;           f += d;
  s.delta = f;        f += b;
  s.lterm = f;        f += b;
  int32_t* i = reinterpret_cast<int32_t*>(f);
  s.treg = i;         i += b;
  s.hreg = i;         i += n;
  s.slot_t = i;       i += P;
  s.slot_h = i;
  return s;
}

// ---------------------------------------------------------------------------------------------
// batch builder: trainDataset.__getitem__ (run_new.py:107-137) for one user. The history stays in
// CSR order (the visit rates are attached by position and the live loop does not shuffle); the
// negatives are make_batch_kernel's (csrc/nais_train.hip): the first n * ng members, in the seeded
// order of [0, P), that are not in the history.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NT_BATCH_THREADS)
new1_make_batch_kernel(const int64_t* __restrict__ indptr, const int64_t* __restrict__ indices,
                       const double* __restrict__ rate, const int64_t* __restrict__ region_of,
                       int64_t user, int64_t n, int64_t P, int ng, uint32_t s1,
                       int64_t* __restrict__ hist, int64_t* __restrict__ hreg,
                       float* __restrict__ vr, int64_t* __restrict__ target,
                       int64_t* __restrict__ treg, float* __restrict__ labels,
                       int32_t* __restrict__ err) {
  __shared__ int32_t scan[NT_BATCH_THREADS / 64];
  __shared__ int64_t base;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t start = indptr[user];
  // workgroup-uniform: a batch that cannot be drawn writes nothing
  if (indptr[user + 1] - start != n || n * ng > P - n) {
    if (tid == 0) atomicOr(err, 1);
    return;
  }
  const int64_t* row = indices + start;
  const uint32_t mP = uint32_t(P);
  const int hP = mP > 1 ? half_bits(mP) : 0;
  for (int64_t i = tid; i < n; i += NT_BATCH_THREADS) {
    const int64_t v = row[i];
    const int64_t rg = (v >= 0 && v < P) ? region_of[v] : -1;
    hist[i] = v;
    hreg[i] = rg;
    vr[i] = float(rate[start + i]);
    target[i * (1 + ng)] = v;
    treg[i * (1 + ng)] = rg;
    labels[i * (1 + ng)] = 1.f;
  }
  if (tid == 0) base = 0;
  __syncthreads();
  const int64_t want = n * ng;
  for (int64_t k0 = 0; k0 < n * (ng + 1); k0 += NT_BATCH_THREADS) {
    const int64_t k = k0 + tid;
    int64_t cand = -1;
    if (k < n * (ng + 1)) {
      cand = mP > 1 ? permute(uint32_t(k), mP, hP, s1) : 0;
      int64_t lo = 0, hi = n;  // binary search in the sorted CSR row
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (row[mid] < cand) lo = mid + 1;
        else hi = mid;
      }
      if (lo < n && row[lo] == cand) cand = -1;
    }
    const bool acc = cand >= 0;
    const unsigned long long bal = __ballot(acc);
    const int before = __popcll(bal & ((1ull << lane) - 1));
    if (lane == 0) scan[w] = __popcll(bal);
    __syncthreads();
    int off = 0, tot = 0;
    for (int q = 0; q < NT_BATCH_THREADS / 64; ++q) {
      if (q < w) off += scan[q];
      tot += scan[q];
    }
    const int64_t pos = base + off + before;
    if (acc && pos < want) {
      const int64_t r = pos / ng, q = pos % ng, o = r * (1 + ng) + 1 + q;
      target[o] = cand;
      treg[o] = region_of[cand];
      labels[o] = 0.f;
    }
    __syncthreads();
    if (tid == 0) base += tot;
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// the rows of the batch: gather, id checks, slots, g
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void new1_rows_gather_kernel(
    NP1T p, const int64_t* __restrict__ hist, const int64_t* __restrict__ hreg,
    const float* __restrict__ vr, const int64_t* __restrict__ target,
    const int64_t* __restrict__ treg, int64_t b, int64_t n, int32_t* __restrict__ st_t,
    int32_t* __restrict__ st_h, int32_t tag, WS w, int32_t* __restrict__ err, int nrowblk) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int d = p.d, half = d >> 1;
  if (int(blockIdx.x) == nrowblk) {   // g[e] = sum_j r_j h_j[e], j ascending (model.py:909)
    for (int e = tid; e < d; e += 256) {
      float s = 0.f;
      for (int64_t j = 0; j < n; ++j) {
        int64_t id = (e < half) ? hist[j] : hreg[j];
        const int64_t lim = (e < half) ? p.P : p.R;
        if (id < 0 || id >= lim) id = 0;   // *err is set by the row's own wave
        const float v = (e < half) ? p.E[id * half + e] : p.Er[id * half + (e - half)];
        s = fmaf(vr[j], v, s);
      }
      w.g[e] = s;
    }
    return;
  }
  const int64_t row = int64_t(blockIdx.x) * 4 + wave;
  if (row >= n + b) return;
  const bool is_h = row < n;
  const int64_t i = is_h ? row : row - n;
  int64_t id = is_h ? hist[i] : target[i];
  int64_t rg = is_h ? hreg[i] : treg[i];
  if (lane == 0) {
    if (id < 0 || id >= p.P) {
      atomicOr(err, 2);
    } else {
      if (atomicExch((is_h ? st_h : st_t) + id, tag) == tag) atomicOr(err, 1);
      (is_h ? w.slot_h : w.slot_t)[id] = int32_t(i);   // a repeat leaves either slot: *err is set
    }
    if (rg < 0 || rg >= p.R) atomicOr(err, 2);
    (is_h ? w.hreg : w.treg)[i] = (rg < 0 || rg >= p.R) ? -1 : int32_t(rg);
  }
  if (id < 0 || id >= p.P) id = 0;
  if (rg < 0 || rg >= p.R) rg = 0;
  float* out = (is_h ? w.H : w.T) + i * d;
  for (int e = lane; e < d; e += 64)
    out[e] = (e < half) ? p.E[id * half + e] : p.Er[rg * half + (e - half)];
}

// ---------------------------------------------------------------------------------------------
// C[m][c] = sum over the segments of sum_k A(k, m) B(k, c)  (+ add[m][c] + rv[m] cv[c])
// A(k, m) = a[k * sak + m * sam], B(k, c) = b[k * sbk + c * sbn]
// ---------------------------------------------------------------------------------------------
struct Seg {
  const float *a, *b;
  int64_t sak, sam, sbk, sbn;
};

struct Job {
  Seg s[2];
  int nseg;
  int M, N, K;             // K is shared by the segments
  float* c;
  int64_t ldc;
  const float* add;        // optional [M][ldadd]
  int64_t ldadd;
  const float *rv, *cv;    // optional rank-one term
  int tile0, ntn;          // first workgroup of the job, its tiles along N
};

struct Jobs {
  Job j[NT_MAXJOBS];
  int njobs;
};

__global__ __launch_bounds__(64 * NT_KW) void new1_gemm_kernel(Jobs js) {
  __shared__ float Lr[NT_KW * 1024];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, ln = lane & 31, hh = lane >> 5;
  int ji = 0;
#pragma unroll
  for (int q = 1; q < NT_MAXJOBS; ++q)
    if (q < js.njobs && int(blockIdx.x) >= js.j[q].tile0) ji = q;
  const Job& jb = js.j[ji];
  const int t = int(blockIdx.x) - jb.tile0;
  const int m0 = (t / jb.ntn) * 32, c0 = (t % jb.ntn) * 32;
  const int m = m0 + ln, c = c0 + ln;
  const bool mok = m < jb.M, cok = c < jb.N;
  const int K = jb.K;
  floatx16 C;
#pragma unroll
  for (int r = 0; r < 16; ++r) C[r] = 0.f;
  for (int sg = 0; sg < jb.nseg; ++sg) {
    const Seg& s = jb.s[sg];
    const float* __restrict__ ap = s.a + int64_t(m) * s.sam;
    const float* __restrict__ bp = s.b + int64_t(c) * s.sbn;
    for (int k0 = 2 * wave; k0 < K; k0 += 2 * NT_KW) {
      const int k = k0 + hh;
      float av = 0.f, bv = 0.f;
      if (k < K) {   // the odd k past K is zero in both operands
        if (mok) av = ap[int64_t(k) * s.sak];
        if (cok) bv = bp[int64_t(k) * s.sbk];
      }
      C = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, C, 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) Lr[wave * 1024 + r * 64 + lane] = C[r];
  __syncthreads();
  for (int o = tid; o < 1024; o += 64 * NT_KW) {
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < NT_KW; ++q) v += Lr[q * 1024 + o];
    const int r = o >> 6, l2 = o & 63;
    const int mm = m0 + crow(r, l2 >> 5), cc = c0 + (l2 & 31);
    if (mm < jb.M && cc < jb.N) {
      if (jb.add) v += jb.add[int64_t(mm) * jb.ldadd + cc];
      if (jb.rv) v = fmaf(jb.rv[mm], jb.cv[cc], v);
      jb.c[int64_t(mm) * jb.ldc + cc] = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// per target row: the softmax-like weights, the prediction, BCELoss and the row's dA, dM
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void new1_rows_loss_kernel(
    int d, float beta, const int64_t* __restrict__ hist, const int64_t* __restrict__ target,
    const float* __restrict__ labels, int64_t b, int64_t n, WS w, int32_t* __restrict__ err,
    float* __restrict__ pred) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = int64_t(blockIdx.x) * 4 + wave;
  if (i >= b) return;
  const int64_t c = target[i];
  float* __restrict__ Ar = w.A + i * n;
  float* __restrict__ Mr = w.M + i * n;
  const float sqd = sqrtf(float(d));
  float S = 0.f, N = 0.f;
  for (int64_t j = lane; j < n; j += 64) {   // exp_A * mask (model.py:899-901)
    const float e = expf(Ar[j] / sqd) * ((hist[j] != c) ? 1.f : 0.f);
    Ar[j] = e;
    S += e;
    N = fmaf(e, Mr[j], N);
  }
  S = wave_sum(S);
  N = wave_sum(N);
  float gd = 0.f;
  for (int e = lane; e < d; e += 64) gd = fmaf(w.T[i * d + e], w.g[e], gd);
  gd = wave_sum(gd);
  const float pw = powf(S, beta);
  const float pr = N / pw + gd;
  const float x = sigmoidf(pr);
  const float y = labels[i];
  // nn.BCELoss after nn.Sigmoid in autograd's composed form (include/nais.h)
  const float lt = -(y * fmaxf(logf(x), -100.f) + (1.f - y) * fmaxf(log1pf(-x), -100.f));
  float dl = (x - y) / fmaxf((1.f - x) * x, 1e-12f);
  dl = dl / float(b);
  dl = dl * (1.f - x) * x;
  if (lane == 0) {
    if (pr != pr) atomicOr(err, 4);   // the reference raises inside BCELoss
    if (pred) pred[i] = x;
    w.delta[i] = dl;
    w.lterm[i] = lt;
  }
  const float sc = dl / pw;             // delta S^-beta
  const float off = beta * N / S;
  for (int64_t j = lane; j < n; j += 64) {
    const float dm = sc * Ar[j];
    const float mv = Mr[j];
    Mr[j] = dm;
    Ar[j] = dm * (mv - off) / sqd;
  }
}

// ---------------------------------------------------------------------------------------------
// torch.optim.Adam, one element (torch/optim/adam.py _single_tensor_adam)
// ---------------------------------------------------------------------------------------------
struct AdamC {
  float wd, b1w, b2, b2w, step_size, bc2s, eps;   // b1w = 1 - beta1, b2w = 1 - beta2
};

__device__ __forceinline__ void adam_elem(float* p, float* m, float* v, float g, const AdamC& a) {
  const float pv = *p;
  if (a.wd != 0.f) g = fmaf(a.wd, pv, g);
  const float mv = fmaf(a.b1w, g - *m, *m);                 // exp_avg.lerp_(grad, 1 - beta1)
  const float vv = fmaf(a.b2w * g, g, *v * a.b2);           // mul_(beta2).addcmul_(g, g, 1 - beta2)
  const float den = sqrtf(vv) / a.bc2s + a.eps;
  *m = mv;
  *v = vv;
  *p = fmaf(-a.step_size, mv / den, pv);                    // addcdiv_(exp_avg, denom, -step_size)
}

struct AdamT {
  float *p, *m, *v;
  const float* g;          // dense gradient (NULL: the rows kind below)
  float* gout;             // optional dense copy of the gradient
  int64_t numel;
};

struct AdamJobs {
  AdamT t[4];              // 0: embed_target (rows kind), 1..3: attn_Q, attn_K, attn_V
};

__global__ __launch_bounds__(256) void new1_adam_dense_kernel(
    AdamJobs js, AdamC a, int half, int d, const int32_t* __restrict__ st_t,
    const int32_t* __restrict__ st_h, int32_t tag, WS w, const int32_t* __restrict__ err) {
  const AdamT& t = js.t[blockIdx.y];
  const bool apply = *err == 0;
  const bool rows = blockIdx.y == 0;
  for (int64_t x = int64_t(blockIdx.x) * 256 + threadIdx.x; x < t.numel;
       x += int64_t(gridDim.x) * 256) {
    float g;
    if (rows) {   // a positive's row receives its dT and its dH share (model.py:872-878)
      const int64_t r = x / half;
      const int e = int(x - r * half);
      g = 0.f;
      if (st_t[r] == tag) g = w.dT[int64_t(w.slot_t[r]) * d + e];
      if (st_h[r] == tag) g += w.dH[int64_t(w.slot_h[r]) * d + e];
    } else {
      g = t.g[x];
    }
    if (t.gout) t.gout[x] = g;
    if (apply) adam_elem(t.p + x, t.m + x, t.v + x, g, a);
  }
}

__global__ __launch_bounds__(256) void new1_adam_region_kernel(
    float* __restrict__ Er, float* __restrict__ m, float* __restrict__ v, float* __restrict__ gout,
    int64_t R, int half, int d, int64_t b, int64_t n, WS w, AdamC a,
    const int32_t* __restrict__ err, double* __restrict__ loss_sum) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t r = int64_t(blockIdx.x) * 4 + wave;
  if (r > R) return;
  if (r == R) {   // the loss: nn.BCELoss's mean, the terms summed in a fixed order
    double s = 0.0;
    for (int64_t i = lane; i < b; i += 64) s += double(w.lterm[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) *loss_sum += s / double(b);
    return;
  }
  float g0 = 0.f, g1 = 0.f;   // half <= 128: elements lane and lane + 64
  const int64_t tot = b + n;
  for (int64_t i0 = 0; i0 < tot; i0 += 64) {
    const int64_t i = i0 + lane;
    int32_t rg = -1;
    if (i < tot) rg = (i < b) ? w.treg[i] : w.hreg[i - b];
    unsigned long long bal = __ballot(int64_t(rg) == r);
    while (bal) {   // wave-uniform: the rows of this region in batch order
      const int q = __ffsll(bal) - 1;
      bal &= bal - 1;
      const int64_t ii = i0 + q;
      const float* src = ((ii < b) ? w.dT + ii * d : w.dH + (ii - b) * d) + half;
      if (lane < half) g0 += src[lane];
      if (lane + 64 < half) g1 += src[lane + 64];
    }
  }
  const bool apply = *err == 0;
  if (lane < half) {
    const int64_t x = r * half + lane;
    if (gout) gout[x] = g0;
    if (apply) adam_elem(Er + x, m + x, v + x, g0, a);
  }
  if (lane + 64 < half) {
    const int64_t x = r * half + lane + 64;
    if (gout) gout[x] = g1;
    if (apply) adam_elem(Er + x, m + x, v + x, g1, a);
  }
}

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

// C [M, N] (ldc) = sum_k A(k, m) B(k, c)
Job job(const float* a, int64_t sak, int64_t sam, const float* b, int64_t sbk, int64_t sbn, int M,
        int N, int K, float* c, int64_t ldc) {
  Job j{};
  j.s[0] = Seg{a, b, sak, sam, sbk, sbn};
  j.nseg = 1;
  j.M = M;
  j.N = N;
  j.K = K;
  j.c = c;
  j.ldc = ldc;
  return j;
}

int launch_jobs(Jobs& js, hipStream_t st) {
  int tiles = 0;
  for (int q = 0; q < js.njobs; ++q) {
    Job& j = js.j[q];
    j.tile0 = tiles;
    j.ntn = (j.N + 31) / 32;
    tiles += ((j.M + 31) / 32) * j.ntn;
  }
  hipLaunchKernelGGL(new1_gemm_kernel, dim3((unsigned)tiles), dim3(64 * NT_KW), 0, st, js);
  return nais_internal_check_launch("new1_gemm_kernel");
}

}  // namespace

extern "C" {

int32_t nais_new1_make_train_batch(const int64_t* indptr, const int64_t* indices,
                                   const double* rate, const int64_t* region_of, int64_t user,
                                   int64_t n, int64_t num_pois, int32_t num_ng, uint64_t seed,
                                   int64_t* hist, int64_t* hist_region, float* visit_rate,
                                   int64_t* target, int64_t* target_region, float* labels,
                                   int32_t* err, void* stream) {
  if (!indptr || !indices || !rate || !region_of || user < 0 || n < 1 || num_ng < 1 ||
      num_pois <= 0)
    return nais_internal_fail(NAIS_E_INVALID, "bad arguments (the history must not be empty)");
  if (num_pois > 0x7fffffffll || n > 0x7fffffffll)
    return nais_internal_fail(NAIS_E_UNSUPPORTED, "num_pois / n must fit 31 bits");
  if (!hist || !hist_region || !visit_rate || !target || !target_region || !labels || !err)
    return nais_internal_fail(NAIS_E_INVALID, "NULL output");
  hipLaunchKernelGGL(new1_make_batch_kernel, dim3(1), dim3(NT_BATCH_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), indptr, indices, rate, region_of, user,
                     n, num_pois, (int)num_ng,
                     mix32(uint32_t(seed >> 32) ^ uint32_t(seed) * 0x9e3779b9u), hist, hist_region,
                     visit_rate, target, target_region, labels, err);
  return nais_internal_check_launch("new1_make_batch_kernel");
}

size_t nais_new1_train_step_workspace_size(const nais_new1_params_t* params, int64_t b, int64_t n) {
  if (!params || b <= 0 || n <= 0) return 0;
  return ws_bytes(b, n, params->embed_dim, params->num_pois);
}

int32_t nais_new1_train_step(const nais_new1_params_t* params, const int64_t* hist,
                             const int64_t* hist_region, const float* visit_rate,
                             const int64_t* target, const int64_t* target_region,
                             const float* labels, int64_t b, int64_t n, double lr,
                             double weight_decay, double beta1, double beta2, double eps,
                             int64_t t, const nais_new1_adam_state_t* state, int32_t* stamp_target,
                             int32_t* stamp_hist, int32_t tag, double* loss_sum, int32_t* err,
                             float* pred, const nais_new1_train_grads_t* grads, void* workspace,
                             size_t workspace_bytes, void* stream) {
  if (int rc = check_params(params)) return rc;
  const nais_new1_params_t& q = *params;
  if (b < 1 || n < 2 || t < 1)
    return nais_internal_fail(NAIS_E_INVALID,
                              "bad shape (b >= 1, t >= 1, and n >= 2: the reference's step raises "
                              "inside BCELoss at n = 1)");
  if (n >= (int64_t(1) << 20) || b >= (int64_t(1) << 24) || b * n >= (int64_t(1) << 31))
    return nais_internal_fail(NAIS_E_UNSUPPORTED, "batch too large");
  if (!hist || !hist_region || !visit_rate || !target || !target_region || !labels || !state ||
      !stamp_target || !stamp_hist || !loss_sum || !err)
    return nais_internal_fail(NAIS_E_INVALID, "NULL pointer");
  const nais_new1_adam_state_t& s = *state;
  if (!s.m_embed_target || !s.v_embed_target || !s.m_embed_region || !s.v_embed_region ||
      !s.m_attn_q || !s.v_attn_q || !s.m_attn_k || !s.v_attn_k || !s.m_attn_v || !s.v_attn_v)
    return nais_internal_fail(NAIS_E_INVALID, "NULL optimiser state");
  const int d = q.embed_dim, half = d >> 1;
  const int64_t P = q.num_pois, R = q.num_regions;
  if (!workspace || workspace_bytes < ws_bytes(b, n, d, P))
    return nais_internal_fail(NAIS_E_WORKSPACE, "workspace missing or too small");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  NP1T p{d,
         P,
         R,
         q.beta,
         const_cast<float*>(q.embed_target),
         const_cast<float*>(q.embed_region),
         const_cast<float*>(q.attn_q),
         const_cast<float*>(q.attn_k),
         const_cast<float*>(q.attn_v)};
  const WS w = carve(workspace, b, n, d, P);
  if (size_t(reinterpret_cast<char*>(w.slot_h + P) - static_cast<char*>(workspace)) >
      ws_bytes(b, n, d, P))   // the carve-up and the size must agree
    return nais_internal_fail(NAIS_E_WORKSPACE, "workspace carve-up exceeds its size");
  const int B = int(b), Nn = int(n);

  const int nrowblk = int((n + b + 3) / 4);
  hipLaunchKernelGGL(new1_rows_gather_kernel, dim3((unsigned)(nrowblk + 1)), dim3(256), 0, st, p,
                     hist, hist_region, visit_rate, target, target_region, b, n, stamp_target,
                     stamp_hist, tag, w, err, nrowblk);
  if (int rc = nais_internal_check_launch("new1_rows_gather_kernel")) return rc;

  Jobs js{};
  // K = H Wk^T, V = H Wv^T, Q = T Wq^T (model.py:879-893)
  js.j[0] = job(w.H, 1, d, p.Wk, 1, d, Nn, d, d, w.K, d);
  js.j[1] = job(w.H, 1, d, p.Wv, 1, d, Nn, d, d, w.V, d);
  js.j[2] = job(w.T, 1, d, p.Wq, 1, d, B, d, d, w.Q, d);
  js.njobs = 3;
  if (int rc = launch_jobs(js, st)) return rc;
  // A = Q Ks with Ks = the key buffer read as [d, n] (model.py:896); M = T V^T
  js = Jobs{};
  js.j[0] = job(w.Q, 1, d, w.K, n, 1, B, Nn, d, w.A, n);
  js.j[1] = job(w.T, 1, d, w.V, 1, d, B, Nn, d, w.M, n);
  js.njobs = 2;
  if (int rc = launch_jobs(js, st)) return rc;

  hipLaunchKernelGGL(new1_rows_loss_kernel, dim3((unsigned)((b + 3) / 4)), dim3(256), 0, st, d,
                     q.beta, hist, target, labels, b, n, w, err, pred);
  if (int rc = nais_internal_check_launch("new1_rows_loss_kernel")) return rc;

  // dQ = dA Ks^T, dTv = dM V, dKs = Q^T dA ([d, n] = dK's buffer), dV = dM^T T, dg = delta^T T
  js = Jobs{};
  js.j[0] = job(w.A, 1, n, w.K, 1, n, B, d, Nn, w.dQ, d);
  js.j[1] = job(w.M, 1, n, w.V, d, 1, B, d, Nn, w.dTv, d);
  js.j[2] = job(w.Q, d, 1, w.A, n, 1, d, Nn, B, w.dK, n);
  js.j[3] = job(w.M, n, 1, w.T, d, 1, Nn, d, B, w.dV, d);
  js.j[4] = job(w.delta, 1, 1, w.T, d, 1, 1, d, B, w.dg, d);
  js.njobs = 5;
  if (int rc = launch_jobs(js, st)) return rc;

  // dT = dQ Wq + dTv + delta g^T;  dH = dK Wk + dV Wv + r dg^T;  the three weight gradients
  js = Jobs{};
  js.j[0] = job(w.dQ, 1, d, p.Wq, d, 1, B, d, d, w.dT, d);
  js.j[0].add = w.dTv;
  js.j[0].ldadd = d;
  js.j[0].rv = w.delta;
  js.j[0].cv = w.g;
  js.j[1] = job(w.dK, 1, d, p.Wk, d, 1, Nn, d, d, w.dH, d);
  js.j[1].s[1] = Seg{w.dV, p.Wv, 1, d, d, 1};
  js.j[1].nseg = 2;
  js.j[1].rv = visit_rate;
  js.j[1].cv = w.dg;
  js.j[2] = job(w.dQ, d, 1, w.T, d, 1, d, d, B, w.dWq, d);
  js.j[3] = job(w.dK, d, 1, w.H, d, 1, d, d, Nn, w.dWk, d);
  js.j[4] = job(w.dV, d, 1, w.H, d, 1, d, d, Nn, w.dWv, d);
  js.njobs = 5;
  if (int rc = launch_jobs(js, st)) return rc;

  // torch.optim.Adam's scalars, formed in double as Python forms them
  AdamC a;
  a.wd = float(weight_decay);
  a.b1w = float(1.0 - beta1);
  a.b2 = float(beta2);
  a.b2w = float(1.0 - beta2);
  a.step_size = float(lr / (1.0 - pow(beta1, double(t))));
  a.bc2s = float(sqrt(1.0 - pow(beta2, double(t))));
  a.eps = float(eps);
  AdamJobs aj{};
  aj.t[0] = AdamT{p.E, s.m_embed_target, s.v_embed_target, nullptr,
                  grads ? grads->embed_target : nullptr, P * half};
  aj.t[1] = AdamT{p.Wq, s.m_attn_q, s.v_attn_q, w.dWq, grads ? grads->attn_q : nullptr,
                  int64_t(d) * d};
  aj.t[2] = AdamT{p.Wk, s.m_attn_k, s.v_attn_k, w.dWk, grads ? grads->attn_k : nullptr,
                  int64_t(d) * d};
  aj.t[3] = AdamT{p.Wv, s.m_attn_v, s.v_attn_v, w.dWv, grads ? grads->attn_v : nullptr,
                  int64_t(d) * d};
  const int64_t big = std::max<int64_t>(P * half, int64_t(d) * d);
  const unsigned grid = unsigned(std::min<int64_t>((big + 255) / 256, 4096));
  hipLaunchKernelGGL(new1_adam_dense_kernel, dim3(grid, 4), dim3(256), 0, st, aj, a, half, d,
                     stamp_target, stamp_hist, tag, w, err);
  if (int rc = nais_internal_check_launch("new1_adam_dense_kernel")) return rc;
  hipLaunchKernelGGL(new1_adam_region_kernel, dim3((unsigned)((R + 1 + 3) / 4)), dim3(256), 0, st,
                     p.Er, s.m_embed_region, s.v_embed_region,
                     grads ? grads->embed_region : nullptr, R, half, d, b, n, w, a, err, loss_sum);
  return nais_internal_check_launch("new1_adam_region_kernel");
}

}  // extern "C"
