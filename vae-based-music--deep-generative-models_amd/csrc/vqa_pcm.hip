// vqa_pcm.hip — fp32 waveform -> int16 PCM (include/vqa.h: vqa_pcm_encode), the inverse of the feed's load
// (vqa_feed.hip, x = i * 2^-15), fused with the crop-and-place step of chunked decoding: each launch takes n samples
// of every row of a decoded chunk, starting at x0, and writes them at o0 of the rows of the full-length output.
// Purely memory-bound: 4 B read and 2 B written per sample, no LDS.
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

}  // namespace vqa

using namespace vqa;

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
  // memory-bound, no LDS: about 2048 workgroups over all rows, each striding over its row's groups
  const long long want = (n + 256ll * 8 - 1) / (256ll * 8), cap = std::max<long long>(1, 2048 / B);
  const dim3 grid((unsigned)std::min(want, cap), (unsigned)B), block(256);
  hipLaunchKernelGGL(pcm_encode_kernel, grid, block, 0, (hipStream_t)stream, x, (long long)ldx, out, (long long)ldo,
                     (long long)x0, (long long)o0, (long long)n, gain, (int*)clipped);
  VQA_LAUNCHED("pcm_encode_kernel");
  return VQA_OK;
}
