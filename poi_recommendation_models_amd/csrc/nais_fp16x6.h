// nais_fp16x6.h -- the split-fp16 arithmetic shared by the catalog kernels (nais_kernels.hip) and
// the on-demand exact refine (nais_pairs.hip): power-of-two scales, the (hi, lo) / (hi, mid, lo)
// f16 splits of an fp32 operand, the six-product 16x16x32 MFMA step and the NaN-keeping ReLU. The
// refine recomputes single pairs of the fp16x6 pair table bit for bit, so both translation units
// take these from one place (not ABI).
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

// 2^e with m * 2^e in [2^13, 2^14) for finite m > 0 (clamped), 1 otherwise
static __device__ __forceinline__ float pow2_scale(float m) {
  if (!(m > 0.f) || !(m < __builtin_huge_valf())) return 1.f;
  const uint32_t bits = __float_as_uint(m);
  int ex = (int)((bits >> 23) & 255u) - 127;
  if (((bits >> 23) & 255u) == 0u) ex = -127;  // subnormal product: maximal (clamped) scale
  int e = 13 - ex;
  e = e < -120 ? -120 : (e > 120 ? 120 : e);
  return __uint_as_float((uint32_t)(e + 127) << 23);
}

// x -> (hi, lo): hi = f16(x) (RNE, v_cvt_pk_f16_f32), lo = f16(x - hi) with the subtraction done
// exactly inside v_fma_mix{lo,hi}_f16 (one instruction per element instead of cvt + sub + cvt).
// The trailing s_nop 1 covers the VALU-write -> MFMA-operand-read hazard that hipcc does not
// pad for inline asm (cdna_hip_programming.md 5.7 item 2).
static __device__ __forceinline__ void split8(const float (&x)[8], half8& hi, half8& lo) {
#pragma unroll
  for (int e = 0; e < 8; ++e) hi[e] = (_Float16)x[e];
  const uint4 hu = *reinterpret_cast<const uint4*>(&hi);
  uint32_t l0, l1, l2, l3;
  asm("v_fma_mixlo_f16 %0, -%4, 1.0, %8 op_sel_hi:[1,0,0]\n\t"
      "v_fma_mixhi_f16 %0, -%4, 1.0, %9 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
      "v_fma_mixlo_f16 %1, -%5, 1.0, %10 op_sel_hi:[1,0,0]\n\t"
      "v_fma_mixhi_f16 %1, -%5, 1.0, %11 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
      "v_fma_mixlo_f16 %2, -%6, 1.0, %12 op_sel_hi:[1,0,0]\n\t"
      "v_fma_mixhi_f16 %2, -%6, 1.0, %13 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
      "v_fma_mixlo_f16 %3, -%7, 1.0, %14 op_sel_hi:[1,0,0]\n\t"
      "v_fma_mixhi_f16 %3, -%7, 1.0, %15 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
      "s_nop 1"
      : "=&v"(l0), "=&v"(l1), "=&v"(l2), "=&v"(l3)
      : "v"(hu.x), "v"(hu.y), "v"(hu.z), "v"(hu.w), "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]),
        "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(x[7]));
  const uint4 lu = make_uint4(l0, l1, l2, l3);
  lo = *reinterpret_cast<const half8*>(&lu);
}

// x -> (hi, mid, lo), x == hi + mid + lo exactly for the scaled operands of this file (33
// significant bits >= fp32's 24; f16 subnormals only below 2^-37 of the scaled maximum):
//   hi = f16(x),  r = x - hi (exact, v_fma_mix_f32),  mid = f16(r),  lo = f16(r - mid) (exact
//   subtraction inside v_fma_mix{lo,hi}_f16). The fp16x6 path multiplies such splits (6 products).
static __device__ __forceinline__ void split8_3(const float (&x)[8], half8& hi, half8& mid, half8& lo) {
#pragma unroll
  for (int e = 0; e < 8; ++e) hi[e] = (_Float16)x[e];
  const uint4 hu = *reinterpret_cast<const uint4*>(&hi);
  const uint32_t hw[4] = {hu.x, hu.y, hu.z, hu.w};
  float r[8];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    asm("v_fma_mix_f32 %0, -%2, 1.0, %3 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mix_f32 %1, -%2, 1.0, %4 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
        : "=&v"(r[2 * q]), "=&v"(r[2 * q + 1])
        : "v"(hw[q]), "v"(x[2 * q]), "v"(x[2 * q + 1]));
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) mid[e] = (_Float16)r[e];
  const uint4 mu = *reinterpret_cast<const uint4*>(&mid);
  uint32_t l0, l1, l2, l3;
  asm("v_fma_mixlo_f16 %0, -%4, 1.0, %8 op_sel_hi:[1,0,0]\n\t"
      "v_fma_mixhi_f16 %0, -%4, 1.0, %9 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
      "v_fma_mixlo_f16 %1, -%5, 1.0, %10 op_sel_hi:[1,0,0]\n\t"
      "v_fma_mixhi_f16 %1, -%5, 1.0, %11 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
      "v_fma_mixlo_f16 %2, -%6, 1.0, %12 op_sel_hi:[1,0,0]\n\t"
      "v_fma_mixhi_f16 %2, -%6, 1.0, %13 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
      "v_fma_mixlo_f16 %3, -%7, 1.0, %14 op_sel_hi:[1,0,0]\n\t"
      "v_fma_mixhi_f16 %3, -%7, 1.0, %15 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
      "s_nop 1"
      : "=&v"(l0), "=&v"(l1), "=&v"(l2), "=&v"(l3)
      : "v"(mu.x), "v"(mu.y), "v"(mu.z), "v"(mu.w), "v"(r[0]), "v"(r[1]), "v"(r[2]), "v"(r[3]),
        "v"(r[4]), "v"(r[5]), "v"(r[6]), "v"(r[7]));
  const uint4 lu = make_uint4(l0, l1, l2, l3);
  lo = *reinterpret_cast<const half8*>(&lu);
}

// NPC split pieces of 8 fp32 values: 2 = (hi, lo) for fp16x3, 3 = (hi, mid, lo) for fp16x6
template <int NPC>
static __device__ __forceinline__ void split_pieces(const float (&x)[8], half8 (&pc)[NPC]) {
  if constexpr (NPC == 2) split8(x, pc[0], pc[1]);
  else split8_3(x, pc[0], pc[1], pc[2]);
}

// ReLU that keeps every NaN, as torch.relu (model.py:71): gfx950's v_maximum3_f32 (IEEE 754-2019
// maximum: NaN propagates, max(-0, +0) = +0), one VALU. (The round-2 form, v_cmp + v_cndmask on
// the float bits, was 1.1 % slower on the pair table: profiles/r3/relu_ab.)
static __device__ __forceinline__ float relu_bits(float v) {
  return __builtin_elementwise_maximum(v, 0.f);   // v_maximum3_f32: IEEE maximum, NaN in -> NaN out
}

static __device__ __forceinline__ floatx4 mfma16n(half8 a, half8 b, floatx4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
// the six fp16x6 products, smallest terms first (as mfma_pieces<3>)
static __device__ __forceinline__ floatx4 mfma16n_pieces(const half8 (&a)[3], const half8 (&b)[3], floatx4 c) {
  c = mfma16n(a[2], b[0], c);
  c = mfma16n(a[1], b[1], c);
  c = mfma16n(a[0], b[2], c);
  c = mfma16n(a[1], b[0], c);
  c = mfma16n(a[0], b[1], c);
  c = mfma16n(a[0], b[0], c);
  return c;
}
