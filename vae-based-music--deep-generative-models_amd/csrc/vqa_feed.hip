// vqa_feed.hip — the device-resident corpus feed (include/vqa.h: vqa_corpus_batch).
//
// The whole training corpus (int16 or fp32 PCM, every track back to back) lives in HBM with a table of window
// starts. One launch per step picks this rank's B windows of the epoch's permutation — from the step counter read
// on the device, so the launch is the same every step and replays inside the train step's hipGraph — and converts
// them to the fp32 (B, T) batch. Purely memory-bound: 2 B (4 B) read and 4 B written per sample.
#include <algorithm>

#include "vqa_common.h"

namespace vqa {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <class S> struct Pcm;
template <> struct Pcm<int16_t> {
  static constexpr int EPC = 8;  // samples per 16-byte chunk
  typedef u32x4 chunk;
  // sample j of the 16 samples held by two consecutive chunks
  template <int J> static __device__ __forceinline__ float get(const chunk& a, const chunk& b) {
    const uint32_t d = (J < 8) ? a[(J & 7) >> 1] : b[(J & 7) >> 1];
    return (float)(int16_t)(uint16_t)(d >> (16 * (J & 1))) * (1.0f / 32768.0f);  // exact in fp32
  }
  static __device__ __forceinline__ float one(const int16_t* p) { return (float)(*p) * (1.0f / 32768.0f); }
};
template <> struct Pcm<float> {
  static constexpr int EPC = 4;
  typedef f32x4 chunk;
  template <int J> static __device__ __forceinline__ float get(const chunk& a, const chunk& b) {
    return (J < 4) ? a[J & 3] : b[J & 3];
  }
  static __device__ __forceinline__ float one(const float* p) { return *p; }
};

// Body of one row for the block-uniform residue R = (first body sample) mod EPC of the source: output group g is the
// EPC samples from t = head + g*EPC, a 16-byte aligned destination; its source samples are the last EPC - R samples
// of the aligned chunk c0 + g and the first R of chunk c0 + g + 1 (not loaded when R = 0: it may lie past the
// corpus). Every register index is a compile-time constant.
template <class S, int R>
__device__ __forceinline__ void feed_body(const typename Pcm<S>::chunk* __restrict__ src, float* __restrict__ dst,
                                          long long ngroups) {
  typedef Pcm<S> P;
  constexpr int E = P::EPC;
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < ngroups; g += (long long)gridDim.x * 256) {
    const typename P::chunk a = src[g];
    typename P::chunk b = a;
    if constexpr (R != 0) b = src[g + 1];
    float* o = dst + g * E;
    *(f32x4*)o = f32x4{P::template get<R + 0>(a, b), P::template get<R + 1>(a, b), P::template get<R + 2>(a, b),
                       P::template get<R + 3>(a, b)};
    if constexpr (E == 8)
      *(f32x4*)(o + 4) = f32x4{P::template get<R + 4>(a, b), P::template get<R + 5>(a, b),
                               P::template get<R + 6>(a, b), P::template get<R + 7>(a, b)};
  }
}

// grid (chunks of T, B), as synth_kernel. Everything up to `ngroups` is computed from kernel arguments, blockIdx and
// two loads at uniform addresses: the window is resolved on the scalar unit once per wave, never per lane (the
// cycle-walking Feistel of perm_index is a scalar loop).
template <class S>
__global__ __launch_bounds__(256) void corpus_batch_kernel(const S* __restrict__ corpus, long long corpus_len,
                                                          const int64_t* __restrict__ starts,
                                                          const int64_t* __restrict__ labels, long long M,
                                                          float* __restrict__ x, int64_t* __restrict__ labels_out,
                                                          int64_t* __restrict__ index_out, int B, long long T,
                                                          uint64_t seed, const int64_t* __restrict__ counter,
                                                          long long step, int rank, int world, int shuffle) {
  typedef Pcm<S> P;
  constexpr int E = P::EPC;
  const int b = blockIdx.y;
  const long long per_step = (long long)B * world, S_ = M / per_step;
  const long long g = step + (counter ? (long long)*counter : 0ll);
  long long epoch = g / S_, pos = g % S_;
  if (pos < 0) {  // a negative counter never indexes the table backwards
    pos += S_;
    epoch -= 1;
  }
  const long long k = (pos * world + rank) * B + b;  // < S_*B*world <= M
  const long long i = shuffle ? perm_index(perm_key(seed, epoch, VQA_FEED_PERM_LEVEL), M, k) : k;
  const long long start = starts[i];
  const bool valid = start >= 0 && corpus_len >= T && start <= corpus_len - T;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (labels_out) labels_out[b] = labels[i];
    if (index_out) index_out[b] = valid ? i : -1;
  }
  float* row = x + (long long)b * T;
  // scalar head up to the first 16-byte aligned output, aligned groups of E samples, scalar tail
  const long long head4 = (long long)((16 - ((uintptr_t)row & 15)) & 15) / 4, head = head4 < T ? head4 : T;
  const long long ngroups = (T - head) / E, tail0 = head + ngroups * E;
  if (!valid) {  // never read: the row is zeros
    if (blockIdx.x == 0 && threadIdx.x < head) row[threadIdx.x] = 0.f;
    if (blockIdx.x == 0 && tail0 + threadIdx.x < T) row[tail0 + threadIdx.x] = 0.f;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < ngroups * (E / 4); q += (long long)gridDim.x * 256)
      *(f32x4*)(row + head + q * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    return;
  }
  const S* win = corpus + start;
  if (blockIdx.x == 0 && threadIdx.x < head) row[threadIdx.x] = P::one(win + threadIdx.x);
  if (blockIdx.x == 0 && tail0 + threadIdx.x < T) row[tail0 + threadIdx.x] = P::one(win + tail0 + threadIdx.x);
  const long long s0 = start + head;  // first body sample; corpus is 16-byte aligned, so chunk s0 / E is too
  const typename P::chunk* src = (const typename P::chunk*)corpus + s0 / E;
  float* dst = row + head;
  switch ((int)(s0 % E)) {
    case 0: feed_body<S, 0>(src, dst, ngroups); break;
    case 1: feed_body<S, 1>(src, dst, ngroups); break;
    case 2: feed_body<S, 2>(src, dst, ngroups); break;
    case 3: feed_body<S, 3>(src, dst, ngroups); break;
    default:
      if constexpr (E == 8) {
        switch ((int)(s0 % E)) {
          case 4: feed_body<S, 4>(src, dst, ngroups); break;
          case 5: feed_body<S, 5>(src, dst, ngroups); break;
          case 6: feed_body<S, 6>(src, dst, ngroups); break;
          default: feed_body<S, 7>(src, dst, ngroups); break;
        }
      }
  }
}

// ---- the code feed (include/vqa.h: vqa_code_batch) -------------------------------------------------------
// The prior's counterpart of the kernel above: the corpus holds VQ codes (int16 or int32) instead of PCM, the batch
// is int64 (what the embedding gather and the cross entropy take), and a conditioned prior gets the window of the
// level above from the same launch. 2 B (4 B) read and 8 B written per code.
typedef int64_t i64x2 __attribute__((ext_vector_type(2)));

// Widening never yields a negative value, whatever the storage holds: int16 is zero-extended, int32 loses its sign bit.
template <class S> struct Code;
template <> struct Code<int16_t> {
  static constexpr int EPC = 8;  // codes per 16-byte chunk
  template <int J> static __device__ __forceinline__ int64_t get(const u32x4& a, const u32x4& b) {
    const uint32_t d = (J < 8) ? a[(J & 7) >> 1] : b[(J & 7) >> 1];
    return (int64_t)(uint16_t)(d >> (16 * (J & 1)));
  }
  static __device__ __forceinline__ int64_t one(const int16_t* p) { return (int64_t)(uint16_t)(*p); }
};
template <> struct Code<int32_t> {
  static constexpr int EPC = 4;
  template <int J> static __device__ __forceinline__ int64_t get(const u32x4& a, const u32x4& b) {
    return (int64_t)(((J < 4) ? a[J & 3] : b[J & 3]) & 0x7fffffffu);
  }
  static __device__ __forceinline__ int64_t one(const int32_t* p) { return (int64_t)((uint32_t)(*p) & 0x7fffffffu); }
};

// As feed_body: output group g is the EPC codes from t = head + g*EPC (a 16-byte aligned destination, EPC/2 stores
// of two int64), taken from the aligned source chunks c0 + g and, when R != 0, c0 + g + 1.
template <class S, int R>
__device__ __forceinline__ void code_body(const u32x4* __restrict__ src, int64_t* __restrict__ dst, long long ngroups) {
  typedef Code<S> P;
  constexpr int E = P::EPC;
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < ngroups; g += (long long)gridDim.x * 256) {
    const u32x4 a = src[g];
    u32x4 b = a;
    if constexpr (R != 0) b = src[g + 1];
    int64_t* o = dst + g * E;
    *(i64x2*)(o + 0) = i64x2{P::template get<R + 0>(a, b), P::template get<R + 1>(a, b)};
    *(i64x2*)(o + 2) = i64x2{P::template get<R + 2>(a, b), P::template get<R + 3>(a, b)};
    if constexpr (E == 8) {
      *(i64x2*)(o + 4) = i64x2{P::template get<R + 4>(a, b), P::template get<R + 5>(a, b)};
      *(i64x2*)(o + 6) = i64x2{P::template get<R + 6>(a, b), P::template get<R + 7>(a, b)};
    }
  }
}

// One row of T codes from corpus + start (valid: the window lies inside the corpus) or T zeros (never read), by all
// the workgroups of the row: a scalar head of 0 or 1 code up to the first 16-byte aligned output (row is 8-byte
// aligned), aligned groups of E codes, a scalar tail of fewer than E.
template <class S>
__device__ __forceinline__ void code_row(const S* __restrict__ corpus, long long start, int64_t* __restrict__ row,
                                         long long T, bool valid) {
  typedef Code<S> P;
  constexpr int E = P::EPC;
  const long long head8 = ((uintptr_t)row & 15) ? 1 : 0, head = head8 < T ? head8 : T;
  const long long ngroups = (T - head) / E, tail0 = head + ngroups * E;
  if (!valid) {
    if (blockIdx.x == 0 && threadIdx.x < head) row[threadIdx.x] = 0;
    if (blockIdx.x == 0 && tail0 + threadIdx.x < T) row[tail0 + threadIdx.x] = 0;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < ngroups * (E / 2); q += (long long)gridDim.x * 256)
      *(i64x2*)(row + head + q * 2) = i64x2{0, 0};
    return;
  }
  const S* win = corpus + start;
  if (blockIdx.x == 0 && threadIdx.x < head) row[threadIdx.x] = P::one(win + threadIdx.x);
  if (blockIdx.x == 0 && tail0 + threadIdx.x < T) row[tail0 + threadIdx.x] = P::one(win + tail0 + threadIdx.x);
  const long long s0 = start + head;  // first body code; the corpus is 16-byte aligned, so chunk s0 / E is too
  const u32x4* src = (const u32x4*)corpus + s0 / E;
  int64_t* dst = row + head;
  switch ((int)(s0 % E)) {
    case 0: code_body<S, 0>(src, dst, ngroups); break;
    case 1: code_body<S, 1>(src, dst, ngroups); break;
    case 2: code_body<S, 2>(src, dst, ngroups); break;
    case 3: code_body<S, 3>(src, dst, ngroups); break;
    default:
      if constexpr (E == 8) {
        switch ((int)(s0 % E)) {
          case 4: code_body<S, 4>(src, dst, ngroups); break;
          case 5: code_body<S, 5>(src, dst, ngroups); break;
          case 6: code_body<S, 6>(src, dst, ngroups); break;
          default: code_body<S, 7>(src, dst, ngroups); break;
        }
      }
  }
}

// grid (chunks of T, B) as corpus_batch_kernel, and the window is resolved the same way (uniform per workgroup). The
// workgroups of item b write its row of z and then, with `upper`, its row of z_upper.
template <class S>
__global__ __launch_bounds__(256) void code_batch_kernel(const S* __restrict__ codes, long long codes_len,
                                                        const S* __restrict__ upper, long long upper_len, int rate,
                                                        const int64_t* __restrict__ starts,
                                                        const int64_t* __restrict__ labels, long long M,
                                                        int64_t* __restrict__ z, int64_t* __restrict__ z_upper,
                                                        int64_t* __restrict__ labels_out,
                                                        int64_t* __restrict__ index_out, int B, long long T,
                                                        uint64_t seed, const int64_t* __restrict__ counter,
                                                        long long step, int rank, int world, int shuffle) {
  const int b = blockIdx.y;
  const long long per_step = (long long)B * world, S_ = M / per_step;
  const long long g = step + (counter ? (long long)*counter : 0ll);
  long long epoch = g / S_, pos = g % S_;
  if (pos < 0) {  // a negative counter never indexes the table backwards
    pos += S_;
    epoch -= 1;
  }
  const long long k = (pos * world + rank) * B + b;  // < S_*B*world <= M
  const long long i = shuffle ? perm_index(perm_key(seed, epoch, VQA_FEED_PERM_LEVEL), M, k) : k;
  const long long start = starts[i];
  const long long Tu = T / rate;
  bool valid = start >= 0 && codes_len >= T && start <= codes_len - T;
  if (upper) valid = valid && start % rate == 0 && upper_len >= Tu && start / rate <= upper_len - Tu;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (labels_out) labels_out[b] = labels[i];
    if (index_out) index_out[b] = valid ? i : -1;
  }
  code_row<S>(codes, start, z + (long long)b * T, T, valid);
  if (upper) code_row<S>(upper, valid ? start / rate : 0, z_upper + (long long)b * Tu, Tu, valid);
}

}  // namespace vqa

using namespace vqa;

extern "C" int64_t vqa_corpus_steps_per_epoch(int64_t M, int B, int world) {
  if (M < 1 || B < 1 || world < 1) return 0;
  return M / ((int64_t)B * world);
}

extern "C" int vqa_corpus_batch(const void* corpus, int64_t corpus_len, int pcm, const int64_t* starts,
                                const int64_t* labels, int64_t M, float* x, int64_t* labels_out, int64_t* index_out,
                                int B, int64_t T, uint64_t seed, const int64_t* counter, int64_t step, int rank,
                                int world, int shuffle, vqa_stream_t stream) {
  VQA_ARG(corpus && starts && x, "corpus_batch: null corpus, starts or x");
  VQA_ARG(B > 0 && T > 0 && M > 0, "corpus_batch: B %d, T %lld and M %lld must be positive", B, (long long)T,
          (long long)M);
  VQA_ARG(B <= 65535, "corpus_batch: B %d above 65535", B);
  VQA_ARG(world >= 1, "corpus_batch: world %d < 1", world);
  VQA_ARG(rank >= 0 && rank < world, "corpus_batch: rank %d outside [0, %d)", rank, world);
  VQA_ARG(M >= (int64_t)B * world, "corpus_batch: M %lld windows < B*world = %lld (no full step in an epoch)",
          (long long)M, (long long)B * world);
  VQA_ARG(pcm == VQA_PCM_I16 || pcm == VQA_PCM_F32, "corpus_batch: pcm %d is neither VQA_PCM_I16 nor VQA_PCM_F32",
          pcm);
  VQA_ARG((uintptr_t)corpus % 16 == 0, "corpus_batch: corpus is not 16-byte aligned");
  VQA_ARG((uintptr_t)x % 4 == 0, "corpus_batch: x is not 4-byte aligned");
  VQA_ARG(!labels_out || labels, "corpus_batch: labels_out given without labels");
  VQA_ARG(step >= 0 && corpus_len >= 0, "corpus_batch: negative step or corpus_len");
  const int epc = pcm == VQA_PCM_I16 ? 8 : 4;
  const unsigned gx = (unsigned)std::min<long long>((T + 256ll * epc - 1) / (256ll * epc), 1024);
  const dim3 grid(gx, (unsigned)B), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (pcm == VQA_PCM_I16) {
    hipLaunchKernelGGL(corpus_batch_kernel<int16_t>, grid, block, 0, s, (const int16_t*)corpus, (long long)corpus_len,
                       starts, labels, (long long)M, x, labels_out, index_out, B, (long long)T, seed, counter,
                       (long long)step, rank, world, shuffle);
  } else {
    hipLaunchKernelGGL(corpus_batch_kernel<float>, grid, block, 0, s, (const float*)corpus, (long long)corpus_len,
                       starts, labels, (long long)M, x, labels_out, index_out, B, (long long)T, seed, counter,
                       (long long)step, rank, world, shuffle);
  }
  VQA_LAUNCHED("corpus_batch_kernel");
  return VQA_OK;
}

extern "C" int vqa_code_batch(const void* codes, int64_t codes_len, const void* upper, int64_t upper_len, int rate,
                              int width, const int64_t* starts, const int64_t* labels, int64_t M, int64_t* z,
                              int64_t* z_upper, int64_t* labels_out, int64_t* index_out, int B, int64_t T,
                              uint64_t seed, const int64_t* counter, int64_t step, int rank, int world, int shuffle,
                              vqa_stream_t stream) {
  VQA_ARG(codes && starts && z, "code_batch: null codes, starts or z");
  VQA_ARG(B > 0 && T > 0 && M > 0, "code_batch: B %d, T %lld and M %lld must be positive", B, (long long)T,
          (long long)M);
  VQA_ARG(B <= 65535, "code_batch: B %d above 65535", B);
  VQA_ARG(rate >= 1, "code_batch: rate %d < 1", rate);
  VQA_ARG(T % rate == 0, "code_batch: T %lld is not a multiple of rate %d", (long long)T, rate);
  VQA_ARG(!upper == !z_upper, "code_batch: upper and z_upper are given together or not at all");
  VQA_ARG(width == VQA_CODE_I16 || width == VQA_CODE_I32,
          "code_batch: width %d is neither VQA_CODE_I16 nor VQA_CODE_I32", width);
  VQA_ARG((uintptr_t)codes % 16 == 0 && (uintptr_t)upper % 16 == 0,
          "code_batch: codes or upper is not 16-byte aligned");
  VQA_ARG((uintptr_t)z % 8 == 0 && (uintptr_t)z_upper % 8 == 0 && (uintptr_t)labels_out % 8 == 0 &&
              (uintptr_t)index_out % 8 == 0,
          "code_batch: z, z_upper, labels_out or index_out is not 8-byte aligned");
  VQA_ARG(world >= 1, "code_batch: world %d < 1", world);
  VQA_ARG(rank >= 0 && rank < world, "code_batch: rank %d outside [0, %d)", rank, world);
  VQA_ARG(M >= (int64_t)B * world, "code_batch: M %lld windows < B*world = %lld (no full step in an epoch)",
          (long long)M, (long long)B * world);
  VQA_ARG(!labels_out || labels, "code_batch: labels_out given without labels");
  VQA_ARG(step >= 0 && codes_len >= 0 && upper_len >= 0, "code_batch: negative step, codes_len or upper_len");
  const int epc = width == VQA_CODE_I16 ? 8 : 4;
  const unsigned gx = (unsigned)std::min<long long>((T + 256ll * epc - 1) / (256ll * epc), 1024);
  const dim3 grid(gx, (unsigned)B), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (width == VQA_CODE_I16) {
    hipLaunchKernelGGL(code_batch_kernel<int16_t>, grid, block, 0, s, (const int16_t*)codes, (long long)codes_len,
                       (const int16_t*)upper, (long long)upper_len, rate, starts, labels, (long long)M, z, z_upper,
                       labels_out, index_out, B, (long long)T, seed, counter, (long long)step, rank, world, shuffle);
  } else {
    hipLaunchKernelGGL(code_batch_kernel<int32_t>, grid, block, 0, s, (const int32_t*)codes, (long long)codes_len,
                       (const int32_t*)upper, (long long)upper_len, rate, starts, labels, (long long)M, z, z_upper,
                       labels_out, index_out, B, (long long)T, seed, counter, (long long)step, rank, world, shuffle);
  }
  VQA_LAUNCHED("code_batch_kernel");
  return VQA_OK;
}
