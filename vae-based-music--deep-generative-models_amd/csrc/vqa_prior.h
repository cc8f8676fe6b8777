// vqa_prior.h — what more than one of the prior's translation units uses (internal); no kernel is defined here.
//   vqa_prior_seqlin.hip : the sequence-linear layers, their weight preparation and weight gradient
//   vqa_prior_attn.hip   : flash (row / prev-row), column and inspection attention
//   vqa_prior_head.hip   : the output head fused with the cross entropy; rowsum
//   vqa_prior_decode.hip : the persistent autoregressive decode kernel with its top-k and nucleus selection
//   vqa_prior.hip        : embeddings and the elementwise glue (colsum, axpy, dropout, scale, teacher forcing)
// Activations are channels-last (rows = N*T, C) in the compute dtype; weights fp32 (Keras layouts); every
// reduction runs in a fixed order (weight gradients as per-workgroup partial rows for vqa_reduce_partials).
#pragma once
#include "vqa_launch.h"
#include "vqa_mfma.h"
#include <algorithm>
#include <math.h>
#include <type_traits>

namespace vqa {

// counter-based uniform in (0, 1): splitmix64 chain over (seed, a, b, c), 24 high bits (oracle/prior_ref.py
// gumbel_uniform restates it)
__host__ __device__ inline float prior_uniform(uint64_t seed, uint64_t a, uint64_t b, uint64_t c) {
  uint64_t h = splitmix64(seed);
  h = splitmix64(h ^ a);
  h = splitmix64(h ^ b);
  h = splitmix64(h ^ c);
  return ((float)(uint32_t)(h >> 40) + 0.5f) * (1.0f / 16777216.0f);
}

constexpr int AHD = 16;  // attention head dim
constexpr float kLog2e = 1.4426950408889634f;

// MFMA traits of the attention kernels (the head's dX / dW reuse mm_rows).
// mm_rows is marked `used`: each unit calls it with one row stride only (attention: AKS, head: hstride), and a
// helper whose every call in the unit passes the same constant has that constant folded into its body before it
// is inlined, which orders the fp32 address arithmetic differently from the form with the stride still a variable
// (attn_fwd / attn_bwd_q / head_bwd_dx / head_bwd_dw <float> came out with other registers, head_bwd_dx with 4
// spills). `used` keeps the helper out of that propagation; the price is one uncalled copy per unit.
template <class T> struct Att;
template <> struct Att<bf16> {
  typedef short s4 __attribute__((ext_vector_type(4)));
  typedef s4 dfrag;  // head dims 4g .. 4g+3 of one row (g = lane >> 4)
  static __device__ __forceinline__ dfrag ld_d(const bf16* row) {
    return *(const s4*)(row + 4 * ((threadIdx.x & 63) >> 4));
  }
  static __device__ __forceinline__ f32x4 mm_d(dfrag a, dfrag b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
  }
  // sum over 32 rows of a row-major tile window (16 columns from `tile`, row stride `stride`): the A operand
  // is the window transposed (lane (col, g) reads rows r0+4g..+3 and r0+16+4g..+3 by ds_read_b64_tr_b16),
  // the B operand the caller's 8 values for the same rows
  __attribute__((used))
  static __device__ __forceinline__ f32x4 mm_rows(const bf16* tile, int stride, int r0, const float (&p)[8], f32x4 c) {
    typedef short v4s __attribute__((ext_vector_type(4)));
    typedef short v8s __attribute__((ext_vector_type(8)));
    const int l = threadIdx.x & 63, li = l & 15, g = l >> 4;
    const bf16* a0 = tile + (r0 + 4 * g + (li >> 2)) * stride + 4 * (li & 3);
    const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)a0);
    const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(a0 + 16 * stride));
    const bf16x8 A = __builtin_bit_cast(bf16x8, (v8s)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
    const bf16x8 B = {(bf16)p[0], (bf16)p[1], (bf16)p[2], (bf16)p[3], (bf16)p[4], (bf16)p[5], (bf16)p[6], (bf16)p[7]};
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, B, c, 0, 0, 0);
  }
};
template <> struct Att<float> {
  typedef f32x4 dfrag;  // element c = head dim 4c + g
  static __device__ __forceinline__ dfrag ld_d(const float* row) {
    const int g = (threadIdx.x & 63) >> 4;
    return f32x4{row[g], row[4 + g], row[8 + g], row[12 + g]};
  }
  static __device__ __forceinline__ f32x4 mm_d(dfrag a, dfrag b, f32x4 c) {
#pragma unroll
    for (int i = 0; i < 4; ++i) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[i], c, 0, 0, 0);
    return c;
  }
  // MFMA j takes rows r0 + 16*(j>>2) + 4g + (j&3) in its K slots g = 0..3
  __attribute__((used))
  static __device__ __forceinline__ f32x4 mm_rows(const float* tile, int stride, int r0, const float (&p)[8], f32x4 c) {
    const int l = threadIdx.x & 63, li = l & 15, g = l >> 4;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      c = __builtin_amdgcn_mfma_f32_16x16x4f32(tile[(r0 + 16 * (j >> 2) + 4 * g + (j & 3)) * stride + li], p[j], c, 0, 0, 0);
    return c;
  }
};

// raw v_exp_f32 (no denormal range handling: probabilities below 2^-126 flush to zero, as in any softmax)
__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }

__device__ __forceinline__ float grp_max(float v) { return xl::max32(xl::max16(v)); }
__device__ __forceinline__ float grp_sum(float v) { return xl::sum32(xl::sum16(v)); }

// host: grid of a grid-stride launch, and the activation dtypes every entry point takes
static int pr_grid(long long work, int per = 256, int cap = 8192) {
  return (int)std::max<long long>(1, std::min<long long>((work + per - 1) / per, cap));
}
static bool pr_dt(int dtype) { return dtype == VQA_F32 || dtype == VQA_BF16; }

}  // namespace vqa
