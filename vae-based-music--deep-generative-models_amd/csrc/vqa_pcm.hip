// vqa_pcm.hip — fp32 waveform -> int16 PCM (include/vqa.h: vqa_pcm_encode), the inverse of the feed's load
// (vqa_feed.hip, x = i * 2^-15), fused with the crop-and-place step of chunked decoding: each launch takes n samples
// of every row of a decoded chunk, starting at x0, and writes them at o0 of the rows of the full-length output.
// Purely memory-bound: 4 B read and 2 B written per sample, no LDS.
// vqa_pcm_splice is the same launch with a second source: the prompt audio p before the seam, x after it and a linear
// cross-fade over the `fade` samples in front of the seam (4 B read per sample outside the fade, 8 B inside).
#include <algorithm>
#include <cmath>

#include "vqa_common.h"

namespace vqa {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// 16-byte load from a 4-byte aligned address: the source of a group follows the destination's alignment, not its own
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

// One sample: v = (x * gain) * 32768 in fp32 (two roundings; the build keeps fma contraction off), rounded half to
// even, NaN -> 0, clamped to the int16 range. `clip` counts the samples whose rounded value lay outside it, NaN too.
__device__ __forceinline__ uint32_t pcm_one(float x, float gain, int& clip) {
  const float v = x * gain * 32768.0f;
  const float r = __builtin_rintf(v);
  clip += !(r >= -32768.0f && r <= 32767.0f);  // false for NaN
  const float c = fminf(fmaxf(r, -32768.0f), 32767.0f);
  return (uint32_t)(uint16_t)(int16_t)(v != v ? 0 : (int)c);
}

__device__ __forceinline__ int wave_sum_int(int v) {  // all 64 lanes active; every lane gets the sum
  v += xl::xor1(v);
  v += xl::xor2(v);
  v += xl::hmirror(v);
  v += xl::mirror(v);
  int a, b;
  xl::pair16(v, a, b);
  v = a + b;
  xl::pair32(v, a, b);
  return a + b;
}

// grid (chunks of n, B), as corpus_batch_kernel. Per row: a scalar head up to the first 16-byte aligned output, groups
// of 8 samples (two 16-byte loads, one 16-byte store), a scalar tail. Only [x0, x0 + n) of a row of x is read and
// only [o0, o0 + n) of a row of out is written.
__global__ __launch_bounds__(256) void pcm_encode_kernel(const float* __restrict__ x, long long ldx,
                                                         int16_t* __restrict__ out, long long ldo, long long x0,
                                                         long long o0, long long n, float gain,
                                                         int* __restrict__ clipped) {
  const int b = blockIdx.y;
  const float* src = x + (long long)b * ldx + x0;
  int16_t* dst = out + (long long)b * ldo + o0;
  const long long head2 = (long long)((16 - ((uintptr_t)dst & 15)) & 15) / 2, head = head2 < n ? head2 : n;
  const long long ngroups = (n - head) / 8, tail0 = head + ngroups * 8;
  int clip = 0;
  if (blockIdx.x == 0 && threadIdx.x < head) dst[threadIdx.x] = (int16_t)pcm_one(src[threadIdx.x], gain, clip);
  if (blockIdx.x == 0 && tail0 + threadIdx.x < n)
    dst[tail0 + threadIdx.x] = (int16_t)pcm_one(src[tail0 + threadIdx.x], gain, clip);
  const float* s = src + head;
  u32x4* d = (u32x4*)(dst + head);
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < ngroups; g += (long long)gridDim.x * 256) {
    const f32x4u a = *(const f32x4u*)(s + g * 8), c = *(const f32x4u*)(s + g * 8 + 4);
    u32x4 o;
    o[0] = pcm_one(a[0], gain, clip) | (pcm_one(a[1], gain, clip) << 16);
    o[1] = pcm_one(a[2], gain, clip) | (pcm_one(a[3], gain, clip) << 16);
    o[2] = pcm_one(c[0], gain, clip) | (pcm_one(c[1], gain, clip) << 16);
    o[3] = pcm_one(c[2], gain, clip) | (pcm_one(c[3], gain, clip) << 16);
    d[g] = o;
  }
  // integer sum over the wave, then one atomic add per wave that clipped anything: the total does not depend on the
  // order the waves arrive in
  clip = wave_sum_int(clip);
  if (clipped && (threadIdx.x & 63) == 0 && clip) atomicAdd(clipped + b, clip);
}

// One spliced sample at j of the launch (absolute t = o0 + j). js = seam - o0 and jf = seam - fade - o0: x from js
// on, p before jf, between them a + (b - a) * w with w = (i + 1) / (fade + 1), i = j - jf — a subtraction, a division,
// a product and a sum, each rounded on its own (-ffp-contract=off, restated here: the test's numpy rule is exact).
// x is not read before jf and p not from js on.
__device__ __forceinline__ float splice_mix(float a, float b, long long i, float fade1) {
#pragma clang fp contract(off)
  const float w = (float)(i + 1) / fade1;
  const float d = b - a;
  const float m = d * w;
  return a + m;
}

__device__ __forceinline__ float splice_one(const float* __restrict__ xs, const float* __restrict__ ps, long long j,
                                            long long js, long long jf, float fade1) {
  if (j >= js) return xs[j];
  if (j < jf) return ps[j];
  return splice_mix(ps[j], xs[j], j - jf, fade1);
}

// pcm_encode_kernel's grid and row plan. Every group of 8 is one of four kinds, the same for all its lanes' samples:
// wholly x (16-byte loads of x), wholly p (of p), wholly inside the fade (of both), or cut by the seam or the fade's
// start (8 scalar picks; at most two such groups in a row).
__global__ __launch_bounds__(256) void pcm_splice_kernel(const float* __restrict__ x, long long ldx,
                                                         const float* __restrict__ p, long long ldp,
                                                         int16_t* __restrict__ out, long long ldo, long long x0,
                                                         long long o0, long long n, long long seam, long long fade,
                                                         float gain, int* __restrict__ clipped) {
  const int b = blockIdx.y;
  const float* xs = x + (long long)b * ldx + x0;
  const float* ps = p + (long long)b * ldp + o0;  // ps[j] = p[row][o0 + j]; dereferenced for o0 + j < seam only
  int16_t* dst = out + (long long)b * ldo + o0;
  const long long js = seam - o0, jf = js - fade;
  const float fade1 = (float)((unsigned long long)fade + 1);
  const long long head2 = (long long)((16 - ((uintptr_t)dst & 15)) & 15) / 2, head = head2 < n ? head2 : n;
  const long long ngroups = (n - head) / 8, tail0 = head + ngroups * 8;
  int clip = 0;
  if (blockIdx.x == 0 && threadIdx.x < head)
    dst[threadIdx.x] = (int16_t)pcm_one(splice_one(xs, ps, threadIdx.x, js, jf, fade1), gain, clip);
  if (blockIdx.x == 0 && tail0 + threadIdx.x < n)
    dst[tail0 + threadIdx.x] = (int16_t)pcm_one(splice_one(xs, ps, tail0 + threadIdx.x, js, jf, fade1), gain, clip);
  u32x4* d = (u32x4*)(dst + head);
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < ngroups; g += (long long)gridDim.x * 256) {
    const long long j0 = head + g * 8;
    f32x4u a, c;
    if (j0 >= js) {
      a = *(const f32x4u*)(xs + j0), c = *(const f32x4u*)(xs + j0 + 4);
    } else if (j0 + 8 <= jf) {
      a = *(const f32x4u*)(ps + j0), c = *(const f32x4u*)(ps + j0 + 4);
    } else if (j0 >= jf && j0 + 8 <= js) {
      const f32x4u pa = *(const f32x4u*)(ps + j0), pc = *(const f32x4u*)(ps + j0 + 4);
      const f32x4u xa = *(const f32x4u*)(xs + j0), xc = *(const f32x4u*)(xs + j0 + 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        a[k] = splice_mix(pa[k], xa[k], j0 + k - jf, fade1);
        c[k] = splice_mix(pc[k], xc[k], j0 + 4 + k - jf, fade1);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        a[k] = splice_one(xs, ps, j0 + k, js, jf, fade1);
        c[k] = splice_one(xs, ps, j0 + 4 + k, js, jf, fade1);
      }
    }
    u32x4 o;
    o[0] = pcm_one(a[0], gain, clip) | (pcm_one(a[1], gain, clip) << 16);
    o[1] = pcm_one(a[2], gain, clip) | (pcm_one(a[3], gain, clip) << 16);
    o[2] = pcm_one(c[0], gain, clip) | (pcm_one(c[1], gain, clip) << 16);
    o[3] = pcm_one(c[2], gain, clip) | (pcm_one(c[3], gain, clip) << 16);
    d[g] = o;
  }
  clip = wave_sum_int(clip);  // as pcm_encode_kernel: one integer atomic per wave that clipped anything
  if (clipped && (threadIdx.x & 63) == 0 && clip) atomicAdd(clipped + b, clip);
}

}  // namespace vqa

using namespace vqa;

// memory-bound, no LDS: about 2048 workgroups over all rows, each striding over its row's groups
static dim3 pcm_grid(int B, long long n) {
  const long long want = (n + 256ll * 8 - 1) / (256ll * 8), cap = std::max<long long>(1, 2048 / B);
  return dim3((unsigned)std::min(want, cap), (unsigned)B);
}

extern "C" int vqa_pcm_encode(const float* x, int64_t ldx, int16_t* out, int64_t ldo, int B, int64_t x0, int64_t o0,
                              int64_t n, float gain, int32_t* clipped, vqa_stream_t stream) {
  VQA_ARG(x && out, "pcm_encode: null x or out");
  VQA_ARG(B > 0 && n > 0, "pcm_encode: B %d and n %lld must be positive", B, (long long)n);
  VQA_ARG(B <= 65535, "pcm_encode: B %d above 65535", B);
  VQA_ARG(x0 >= 0 && o0 >= 0, "pcm_encode: negative x0 %lld or o0 %lld", (long long)x0, (long long)o0);
  VQA_ARG(x0 <= ldx && n <= ldx - x0, "pcm_encode: x0 %lld + n %lld exceeds the row of ldx %lld samples",
          (long long)x0, (long long)n, (long long)ldx);
  VQA_ARG(o0 <= ldo && n <= ldo - o0, "pcm_encode: o0 %lld + n %lld exceeds the row of ldo %lld samples",
          (long long)o0, (long long)n, (long long)ldo);
  VQA_ARG((uintptr_t)x % 4 == 0, "pcm_encode: x is not 4-byte aligned");
  VQA_ARG((uintptr_t)out % 2 == 0, "pcm_encode: out is not 2-byte aligned");
  VQA_ARG((uintptr_t)clipped % 4 == 0, "pcm_encode: clipped is not 4-byte aligned");
  VQA_ARG(std::isfinite(gain) && gain >= 0.0f, "pcm_encode: gain %g is not finite and >= 0", (double)gain);
  const dim3 grid = pcm_grid(B, n), block(256);
  hipLaunchKernelGGL(pcm_encode_kernel, grid, block, 0, (hipStream_t)stream, x, (long long)ldx, out, (long long)ldo,
                     (long long)x0, (long long)o0, (long long)n, gain, (int*)clipped);
  VQA_LAUNCHED("pcm_encode_kernel");
  return VQA_OK;
}

extern "C" int vqa_pcm_splice(const float* x, int64_t ldx, const float* p, int64_t ldp, int16_t* out, int64_t ldo,
                              int B, int64_t x0, int64_t o0, int64_t n, int64_t seam, int64_t fade, float gain,
                              int32_t* clipped, vqa_stream_t stream) {
  VQA_ARG(x && out, "pcm_splice: null x or out");
  VQA_ARG(p, "pcm_splice: null p");
  VQA_ARG(B > 0 && n > 0, "pcm_splice: B %d and n %lld must be positive", B, (long long)n);
  VQA_ARG(B <= 65535, "pcm_splice: B %d above 65535", B);
  VQA_ARG(x0 >= 0 && o0 >= 0, "pcm_splice: negative x0 %lld or o0 %lld", (long long)x0, (long long)o0);
  VQA_ARG(x0 <= ldx && n <= ldx - x0, "pcm_splice: x0 %lld + n %lld exceeds the row of ldx %lld samples",
          (long long)x0, (long long)n, (long long)ldx);
  VQA_ARG(o0 <= ldo && n <= ldo - o0, "pcm_splice: o0 %lld + n %lld exceeds the row of ldo %lld samples",
          (long long)o0, (long long)n, (long long)ldo);
  VQA_ARG(seam >= 0, "pcm_splice: negative seam %lld", (long long)seam);
  VQA_ARG(fade >= 0 && fade <= seam, "pcm_splice: fade %lld outside [0, seam %lld]", (long long)fade,
          (long long)seam);
  VQA_ARG(ldp >= std::min<int64_t>(seam, o0 + n), "pcm_splice: ldp %lld is short of min(seam %lld, o0 + n %lld)",
          (long long)ldp, (long long)seam, (long long)(o0 + n));
  VQA_ARG((uintptr_t)x % 4 == 0, "pcm_splice: x is not 4-byte aligned");
  VQA_ARG((uintptr_t)p % 4 == 0, "pcm_splice: p is not 4-byte aligned");
  VQA_ARG((uintptr_t)out % 2 == 0, "pcm_splice: out is not 2-byte aligned");
  VQA_ARG((uintptr_t)clipped % 4 == 0, "pcm_splice: clipped is not 4-byte aligned");
  VQA_ARG(std::isfinite(gain) && gain >= 0.0f, "pcm_splice: gain %g is not finite and >= 0", (double)gain);
  const dim3 grid = pcm_grid(B, n), block(256);
  hipLaunchKernelGGL(pcm_splice_kernel, grid, block, 0, (hipStream_t)stream, x, (long long)ldx, p, (long long)ldp, out,
                     (long long)ldo, (long long)x0, (long long)o0, (long long)n, (long long)seam, (long long)fade, gain,
                     (int*)clipped);
  VQA_LAUNCHED("pcm_splice_kernel");
  return VQA_OK;
}
