// vqa_prior.hip — the factorized-attention prior's embeddings and elementwise glue (gfx950). The other kernel
// families are in vqa_prior_seqlin.hip, vqa_prior_attn.hip, vqa_prior_head.hip and vqa_prior_decode.hip; what they
// share is in vqa_prior.h.
//
// Replaces (reference file:line):
//   src/autoregressive/autoregressive_fmha.py:119-158   FMHABasedAutoregressiveModel.call
//       x_embedding * sqrt(d_model) + PositionalEmbedding, dropout, (+ x_cond)   -> prior_embed_fwd
//   autoregressive.py:189-212, prior.py:272-300          teacher forcing                   -> tf_mix
#include "vqa_prior.h"

namespace vqa {

// ---------------------------------------------------------------------------------------------------
// embeddings (autoregressive_fmha.py:119-151): x = table[tok] (row 0 replaced by y_cond when given) * scale
// + pos[t]; dropout; + x_cond. One thread per 4 channels.
constexpr unsigned long long kEmbDropSalt = 0x454d42ull;  // VQA_EMB_DROPOUT_SALT (vqa.h)

struct EmbArgs {
  const float* table;
  const float* pos;
  const int64_t* tok;
  const float* ycond;  // (N, W) or null
  const void* xcond;   // (N, T, W) activation dtype or null
  void* out;
  long long rows;
  int T, W, bins;
  float scale, rate;
  unsigned long long seed;
  const int64_t* ctr;  // optional device step counter mixed into the seed (advances under graph replay)
  long long off;       // global flat index of out[0] (data parallel: rank * N*T*W) — the dropout mask's key
};

__device__ __forceinline__ unsigned long long seed_at(unsigned long long seed, const int64_t* ctr) {
  return ctr ? seed ^ splitmix64((uint64_t)*ctr) : seed;
}

template <class T>
__global__ __launch_bounds__(256) void prior_embed_kernel(EmbArgs a) {
  const long long total = a.rows * (a.W / 4);
  const unsigned long long seed = seed_at(a.seed, a.ctr);
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const long long r = e / (a.W / 4);
    const int c = (int)(e - r * (a.W / 4)) * 4, t = (int)(r % a.T);
    const long long n = r / a.T;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (a.ycond && t == 0) {
      v = *(const f32x4*)(a.ycond + n * a.W + c);
    } else {
      const int64_t k = a.tok[r];
      if (k >= 0 && k < a.bins) v = *(const f32x4*)(a.table + k * a.W + c);
    }
    v = v * a.scale;
    v = v + *(const f32x4*)(a.pos + (long long)t * a.W + c);
    if (a.rate > 0.f) {
      // the mask of dropout_kernel over the flat (N, T, W) index with salt kEmbDropSalt: the backward is
      // vqa_dropout on the gradient with the same (seed, salt, counter)
      const float ks = 1.0f / (1.0f - a.rate);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        v[i] = prior_uniform(seed, kEmbDropSalt, (uint64_t)(a.off + r * a.W + c + i), 0) >= a.rate ? v[i] * ks : 0.f;
    }
    if (a.xcond) v = v + ld4((const T*)a.xcond + r * a.W + c);
    st4((T*)a.out + r * a.W + c, v);
  }
}

// out[r][c] (+)= sum_{n < nout} x[n * ostride + r * C + c], fixed order over n (fp32 out)
template <class T>
__global__ __launch_bounds__(256) void colsum_kernel(const T* x, float* out, int nout, long long ostride, long long inner,
                                                    int accumulate) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < inner; e += (long long)gridDim.x * 256) {
    float s = 0.f;
    for (int n = 0; n < nout; ++n) s += ld(x + n * ostride + e);
    out[e] = accumulate ? out[e] + s : s;
  }
}

template <class T>
__global__ __launch_bounds__(256) void axpy_kernel(const T* x, const T* y, T* z, long long n) {
  for (long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; e < n; e += (long long)gridDim.x * 1024) {
    if (e + 4 <= n) {
      st4(z + e, ld4(x + e) + ld4(y + e));
    } else {
      for (long long i = e; i < n; ++i) st(z + i, ld(x + i) + ld(y + i));
    }
  }
}

// keras Dropout(rate): x * (1 / (1 - rate)) where u >= rate, else 0 (the same mask on the gradient); the mask
// is keyed on the global flat index off + e (data parallel: each rank passes its shard's first index)
template <class T>
__global__ __launch_bounds__(256) void dropout_kernel(T* x, long long n, float rate, unsigned long long seed0,
                                                     unsigned long long salt, long long off, const int64_t* ctr) {
  const float ks = 1.0f / (1.0f - rate);
  const unsigned long long seed = seed_at(seed0, ctr);
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256)
    st(x + e, prior_uniform(seed, salt, (uint64_t)(off + e), 0) >= rate ? ld(x + e) * ks : 0.f);
}

__global__ __launch_bounds__(256) void scale_f32_kernel(float* x, long long n, float s) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) x[e] *= s;
}

// prior.py:262-290: latent_input = [start, codes[:-1]]; pred = [start, argmax[:-1]];
// out = mask ? pred : latent_input with mask = explicit (uint8) or uniform(seed, step, row) < rate
__global__ __launch_bounds__(256) void tf_mix_kernel(const int64_t* codes, const int64_t* amax, const uint8_t* mask,
                                                    int64_t* out, long long rows, int T, int64_t start, float rate,
                                                    unsigned long long seed, unsigned long long step0,
                                                    long long row_offset, const int64_t* ctr) {
  const unsigned long long step = step0 + (ctr ? (unsigned long long)*ctr : 0ull);
  for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < rows; r += (long long)gridDim.x * 256) {
    const int t = (int)(r % T);
    const int64_t latent = t == 0 ? start : codes[r - 1];
    bool m = false;
    if (amax) m = mask ? mask[r] != 0 : prior_uniform(seed, 0x5446ull, step, (uint64_t)(r + row_offset)) < rate;
    out[r] = m ? (t == 0 ? start : amax[r - 1]) : latent;
  }
}

}  // namespace vqa

using namespace vqa;

extern "C" int vqa_prior_embed_fwd(const float* table, const float* pos, const int64_t* tokens, const float* ycond,
                                   const void* xcond, void* out, int N, int T, int W, int bins, float scale, float rate,
                                   uint64_t seed, int64_t elem_offset, const int64_t* counter, int dtype,
                                   vqa_stream_t stream) {
  VQA_ARG(table && pos && tokens && out && N > 0 && T > 0 && W > 0 && W % 4 == 0 && bins > 0 && rate >= 0.f &&
              rate < 1.f && elem_offset >= 0, "prior_embed_fwd: bad arguments");
  VQA_ARG(pr_dt(dtype), "prior_embed_fwd: unknown dtype %d", dtype);
  EmbArgs a{table, pos, tokens, ycond, xcond, out, (long long)N * T, T, W, bins, scale, rate, seed, counter,
            (long long)elem_offset};
  const unsigned g = pr_grid(a.rows * (W / 4));
  if (dtype == VQA_BF16) hipLaunchKernelGGL(prior_embed_kernel<bf16>, dim3(g), dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(prior_embed_kernel<float>, dim3(g), dim3(256), 0, (hipStream_t)stream, a);
  VQA_LAUNCHED("prior_embed_kernel");
  return VQA_OK;
}

extern "C" int vqa_colsum(const void* x, float* out, int nout, int64_t ostride, int64_t inner, int accumulate,
                          int dtype, vqa_stream_t stream) {
  VQA_ARG(x && out && nout > 0 && inner > 0 && pr_dt(dtype), "colsum: bad arguments");
  const unsigned g = pr_grid(inner);
  if (dtype == VQA_BF16)
    hipLaunchKernelGGL(colsum_kernel<bf16>, dim3(g), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, out, nout,
                       (long long)ostride, (long long)inner, accumulate);
  else
    hipLaunchKernelGGL(colsum_kernel<float>, dim3(g), dim3(256), 0, (hipStream_t)stream, (const float*)x, out, nout,
                       (long long)ostride, (long long)inner, accumulate);
  VQA_LAUNCHED("colsum_kernel");
  return VQA_OK;
}

extern "C" int vqa_axpy(const void* x, const void* y, void* z, int64_t n, int dtype, vqa_stream_t stream) {
  VQA_ARG(x && y && z && n > 0 && pr_dt(dtype), "axpy: bad arguments");
  const unsigned g = pr_grid((n + 3) / 4);
  if (dtype == VQA_BF16)
    hipLaunchKernelGGL(axpy_kernel<bf16>, dim3(g), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, (const bf16*)y,
                       (bf16*)z, (long long)n);
  else
    hipLaunchKernelGGL(axpy_kernel<float>, dim3(g), dim3(256), 0, (hipStream_t)stream, (const float*)x,
                       (const float*)y, (float*)z, (long long)n);
  VQA_LAUNCHED("axpy_kernel");
  return VQA_OK;
}

extern "C" int vqa_dropout(void* x, int64_t n, float rate, uint64_t seed, uint64_t salt, int64_t elem_offset,
                           const int64_t* counter, int dtype, vqa_stream_t stream) {
  VQA_ARG(x && n > 0 && rate >= 0.f && rate < 1.f && elem_offset >= 0 && pr_dt(dtype), "dropout: bad arguments");
  if (rate == 0.f) return VQA_OK;
  const unsigned g = pr_grid(n);
  if (dtype == VQA_BF16)
    hipLaunchKernelGGL(dropout_kernel<bf16>, dim3(g), dim3(256), 0, (hipStream_t)stream, (bf16*)x, (long long)n, rate,
                       (unsigned long long)seed, (unsigned long long)salt, (long long)elem_offset, counter);
  else
    hipLaunchKernelGGL(dropout_kernel<float>, dim3(g), dim3(256), 0, (hipStream_t)stream, (float*)x, (long long)n,
                       rate, (unsigned long long)seed, (unsigned long long)salt, (long long)elem_offset, counter);
  VQA_LAUNCHED("dropout_kernel");
  return VQA_OK;
}

extern "C" int vqa_scale_f32(float* x, int64_t n, float s, vqa_stream_t stream) {
  VQA_ARG(x && n > 0, "scale_f32: bad arguments");
  hipLaunchKernelGGL(scale_f32_kernel, dim3(pr_grid(n)), dim3(256), 0, (hipStream_t)stream, x, (long long)n, s);
  VQA_LAUNCHED("scale_f32_kernel");
  return VQA_OK;
}

extern "C" int vqa_tf_mix(const int64_t* codes, const int64_t* amax, const uint8_t* mask, int64_t* out, int N, int T,
                          int64_t start, float rate, uint64_t seed, uint64_t step, int64_t row_offset,
                          const int64_t* counter, vqa_stream_t stream) {
  VQA_ARG(codes && out && N > 0 && T > 0 && (!mask || amax), "tf_mix: bad arguments");
  const long long rows = (long long)N * T;
  hipLaunchKernelGGL(tf_mix_kernel, dim3(pr_grid(rows)), dim3(256), 0, (hipStream_t)stream, codes, amax, mask, out,
                     rows, T, start, rate, (unsigned long long)seed, (unsigned long long)step, (long long)row_offset, counter);
  VQA_LAUNCHED("tf_mix_kernel");
  return VQA_OK;
}
