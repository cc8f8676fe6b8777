// vqa_feed.hip — the device-resident corpus feeds (include/vqa.h: vqa_corpus_batch, vqa_code_batch).
//
// A whole training corpus lives in HBM — int16 or fp32 PCM for the VQ-VAE, int16 or int32 VQ codes for the prior,
// every track back to back — with a table of window starts. One launch per step picks this rank's B windows of the
// epoch's permutation — from the step counter read on the device, so the launch is the same every step and replays
// inside the train step's hipGraph — and converts them to the (B, T) batch: fp32 from PCM, int64 (what the embedding
// gather and the cross entropy take) from codes, where a conditioned prior gets the window of the level above from
// the same launch. Purely memory-bound: 2 B (4 B) read and 4 B (8 B) written per element.
#include <algorithm>

#include "vqa_common.h"

namespace vqa {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef int64_t i64x2 __attribute__((ext_vector_type(2)));

// lane J of the 16 16-bit (8 32-bit) values held by two consecutive 16-byte chunks
template <int J> __device__ __forceinline__ uint16_t lane16(const u32x4& a, const u32x4& b) {
  const uint32_t d = (J < 8) ? a[(J & 7) >> 1] : b[(J & 7) >> 1];
  return (uint16_t)(d >> (16 * (J & 1)));
}
template <int J, class C> __device__ __forceinline__ auto lane32(const C& a, const C& b) {
  return (J < 4) ? a[J & 3] : b[J & 3];
}

// How a stored S becomes a batch D: EPC source elements per 16-byte `chunk`, `vec` the 16-byte store of D, get<J>
// element J of two consecutive chunks, one(p) a single element. Widening a code never yields a negative value,
// whatever the storage holds: int16 is zero-extended, int32 loses its sign bit.
template <class S, class D> struct Elem;
template <> struct Elem<int16_t, float> {
  static constexpr int EPC = 8;
  typedef u32x4 chunk;
  typedef f32x4 vec;
  static __device__ __forceinline__ float cvt(uint16_t v) { return (float)(int16_t)v * (1.0f / 32768.0f); }  // exact
  template <int J> static __device__ __forceinline__ float get(const u32x4& a, const u32x4& b) {
    return cvt(lane16<J>(a, b));
  }
  static __device__ __forceinline__ float one(const int16_t* p) { return cvt((uint16_t)*p); }
};
template <> struct Elem<float, float> {
  static constexpr int EPC = 4;
  typedef f32x4 chunk;
  typedef f32x4 vec;
  template <int J> static __device__ __forceinline__ float get(const f32x4& a, const f32x4& b) {
    return lane32<J>(a, b);
  }
  static __device__ __forceinline__ float one(const float* p) { return *p; }
};
template <> struct Elem<int16_t, int64_t> {
  static constexpr int EPC = 8;
  typedef u32x4 chunk;
  typedef i64x2 vec;
  template <int J> static __device__ __forceinline__ int64_t get(const u32x4& a, const u32x4& b) {
    return (int64_t)lane16<J>(a, b);
  }
  static __device__ __forceinline__ int64_t one(const int16_t* p) { return (int64_t)(uint16_t)(*p); }
};
template <> struct Elem<int32_t, int64_t> {
  static constexpr int EPC = 4;
  typedef u32x4 chunk;
  typedef i64x2 vec;
  template <int J> static __device__ __forceinline__ int64_t get(const u32x4& a, const u32x4& b) {
    return (int64_t)(lane32<J>(a, b) & 0x7fffffffu);
  }
  static __device__ __forceinline__ int64_t one(const int32_t* p) { return (int64_t)((uint32_t)(*p) & 0x7fffffffu); }
};

// one 16-byte store's worth of output elements from element J on
template <class P, int J, class C> __device__ __forceinline__ typename P::vec feed_pack(const C& a, const C& b) {
  if constexpr (sizeof(typename P::vec) == 4 * sizeof(P::template get<J>(a, b)))  // f32x4, else i64x2
    return {P::template get<J>(a, b), P::template get<J + 1>(a, b), P::template get<J + 2>(a, b),
            P::template get<J + 3>(a, b)};
  else
    return {P::template get<J>(a, b), P::template get<J + 1>(a, b)};
}

// Body of one row for the block-uniform residue R = (first body element) mod EPC of the source: output group g is the
// EPC elements from t = head + g*EPC, a 16-byte aligned destination written by EPC * sizeof(D) / 16 stores; its
// source elements are the last EPC - R elements of the aligned chunk c0 + g and the first R of chunk c0 + g + 1 (not
// loaded when R = 0: it may lie past the corpus). Every register index is a compile-time constant.
template <class P, int R, class D>
__device__ __forceinline__ void feed_body(const typename P::chunk* __restrict__ src, D* __restrict__ dst,
                                          long long ngroups) {
  typedef typename P::vec vec;
  typedef typename P::chunk chunk;
  constexpr int E = P::EPC, V = 16 / sizeof(D), NV = E / V;  // elements per store, stores per group: 2, 1, 4, 2
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < ngroups; g += (long long)gridDim.x * 256) {
    const chunk a = src[g];
    chunk b = a;
    if constexpr (R != 0) b = src[g + 1];
    D* o = dst + g * E;
    *(vec*)o = feed_pack<P, R>(a, b);
    if constexpr (NV >= 2) *(vec*)(o + V) = feed_pack<P, R + V>(a, b);
    if constexpr (NV == 4) {
      *(vec*)(o + 2 * V) = feed_pack<P, R + 2 * V>(a, b);
      *(vec*)(o + 3 * V) = feed_pack<P, R + 3 * V>(a, b);
    }
  }
}

// One row of T elements from corpus + start (valid: the window lies inside the corpus) or T zeros (never read), by
// all the workgroups of the row: a scalar head up to the first 16-byte aligned output (row is aligned to a D),
// aligned groups of E elements, a scalar tail of fewer than E.
template <class S, class D>
__device__ __forceinline__ void feed_row(const S* __restrict__ corpus, long long start, D* __restrict__ row,
                                         long long T, bool valid) {
  typedef Elem<S, D> P;
  typedef typename P::vec vec;
  constexpr int E = P::EPC, V = 16 / sizeof(D);
  const long long head16 = (long long)((16 - ((uintptr_t)row & 15)) & 15) / (long long)sizeof(D);
  const long long head = head16 < T ? head16 : T, ngroups = (T - head) / E, tail0 = head + ngroups * E;
  if (!valid) {
    if (blockIdx.x == 0 && threadIdx.x < head) row[threadIdx.x] = 0;
    if (blockIdx.x == 0 && tail0 + threadIdx.x < T) row[tail0 + threadIdx.x] = 0;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < ngroups * (E / V); q += gridDim.x * 256ll)
      *(vec*)(row + head + q * V) = vec{};
    return;
  }
  const S* win = corpus + start;
  if (blockIdx.x == 0 && threadIdx.x < head) row[threadIdx.x] = P::one(win + threadIdx.x);
  if (blockIdx.x == 0 && tail0 + threadIdx.x < T) row[tail0 + threadIdx.x] = P::one(win + tail0 + threadIdx.x);
  const long long s0 = start + head;  // first body element, >= 0; the corpus is 16-byte aligned, so chunk s0 / E is too
  const typename P::chunk* src = (const typename P::chunk*)corpus + s0 / E;
  D* dst = row + head;
  switch ((int)(s0 & (E - 1))) {  // below E: with E = 4 the cases from 4 on are dead code and compiled away
    case 0: feed_body<P, 0>(src, dst, ngroups); break;
    case 1: feed_body<P, 1>(src, dst, ngroups); break;
    case 2: feed_body<P, 2>(src, dst, ngroups); break;
    case 3: feed_body<P, 3>(src, dst, ngroups); break;
    case 4: feed_body<P, 4>(src, dst, ngroups); break;
    case 5: feed_body<P, 5>(src, dst, ngroups); break;
    case 6: feed_body<P, 6>(src, dst, ngroups); break;
    default: feed_body<P, 7>(src, dst, ngroups); break;
  }
}

// The window of item b = blockIdx.y (include/vqa.h: g, S, epoch, pos, slot k, permutation). Everything here is
// computed from kernel arguments, blockIdx and two loads at uniform addresses: the window is resolved on the scalar
// unit once per wave, never per lane (the cycle-walking Feistel of perm_index is a scalar loop).
struct Window {
  long long i, start;
};
__device__ __forceinline__ Window feed_window(const int64_t* __restrict__ starts, long long M, int B, uint64_t seed,
                                              const int64_t* __restrict__ counter, long long step, int rank, int world,
                                              int shuffle) {
  const long long per_step = (long long)B * world, S_ = M / per_step;
  const long long g = step + (counter ? (long long)*counter : 0ll);
  long long epoch = g / S_, pos = g % S_;
  if (pos < 0) {  // a negative counter never indexes the table backwards
    pos += S_;
    epoch -= 1;
  }
  const long long k = (pos * world + rank) * B + blockIdx.y;  // < S_*B*world <= M
  const long long i = shuffle ? perm_index(perm_key(seed, epoch, VQA_FEED_PERM_LEVEL), M, k) : k;
  return {i, starts[i]};
}

// grid (chunks of T, B), as synth_kernel
template <class S>
__global__ __launch_bounds__(256) void corpus_batch_kernel(const S* __restrict__ corpus, long long corpus_len,
                                                          const int64_t* __restrict__ starts,
                                                          const int64_t* __restrict__ labels, long long M,
                                                          float* __restrict__ x, int64_t* __restrict__ labels_out,
                                                          int64_t* __restrict__ index_out, int B, long long T,
                                                          uint64_t seed, const int64_t* __restrict__ counter,
                                                          long long step, int rank, int world, int shuffle) {
  const int b = blockIdx.y;
  const Window w = feed_window(starts, M, B, seed, counter, step, rank, world, shuffle);
  const bool valid = w.start >= 0 && corpus_len >= T && w.start <= corpus_len - T;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (labels_out) labels_out[b] = labels[w.i];
    if (index_out) index_out[b] = valid ? w.i : -1;
  }
  feed_row(corpus, w.start, x + (long long)b * T, T, valid);
}

// The same grid. The workgroups of item b write its row of z and then, with `upper`, its row of z_upper.
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
  const Window w = feed_window(starts, M, B, seed, counter, step, rank, world, shuffle);
  const long long Tu = T / rate;
  bool valid = w.start >= 0 && codes_len >= T && w.start <= codes_len - T;
  if (upper) valid = valid && w.start % rate == 0 && upper_len >= Tu && w.start / rate <= upper_len - Tu;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (labels_out) labels_out[b] = labels[w.i];
    if (index_out) index_out[b] = valid ? w.i : -1;
  }
  feed_row(codes, w.start, z + (long long)b * T, T, valid);
  if (upper) feed_row(upper, valid ? w.start / rate : 0, z_upper + (long long)b * Tu, Tu, valid);
}

// The argument checks the two feeds share; `op` starts the message.
static int feed_args(const char* op, int B, int64_t T, int64_t M, int rank, int world, const void* labels,
                     const void* labels_out) {
  VQA_ARG(B > 0 && T > 0 && M > 0, "%s: B %d, T %lld and M %lld must be positive", op, B, (long long)T, (long long)M);
  VQA_ARG(B <= 65535, "%s: B %d above 65535", op, B);
  VQA_ARG(world >= 1, "%s: world %d < 1", op, world);
  VQA_ARG(rank >= 0 && rank < world, "%s: rank %d outside [0, %d)", op, rank, world);
  VQA_ARG(M >= (int64_t)B * world, "%s: M %lld windows < B*world = %lld (no full step in an epoch)", op, (long long)M,
          (long long)B * world);
  VQA_ARG(!labels_out || labels, "%s: labels_out given without labels", op);
  return VQA_OK;
}

// grid (ceil(T / (256 * EPC)) up to 1024, B) x 256 threads. launch(S(), grid) starts the kernel of storage type S:
// int16 (EPC 8) when `narrow`, else the 4-byte S4 (EPC 4).
template <class S4, class F> static int feed_launch(const char* kernel, bool narrow, int B, int64_t T, F launch) {
  const int epc = narrow ? 8 : 4;
  const dim3 grid((unsigned)std::min<long long>((T + 256ll * epc - 1) / (256ll * epc), 1024), (unsigned)B);
  if (narrow) launch(int16_t(), grid);
  else launch(S4(), grid);
  VQA_LAUNCHED(kernel);
  return VQA_OK;
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
  if (int rc = feed_args("corpus_batch", B, T, M, rank, world, labels, labels_out)) return rc;
  VQA_ARG(pcm == VQA_PCM_I16 || pcm == VQA_PCM_F32, "corpus_batch: pcm %d is neither VQA_PCM_I16 nor VQA_PCM_F32",
          pcm);
  VQA_ARG((uintptr_t)corpus % 16 == 0, "corpus_batch: corpus is not 16-byte aligned");
  VQA_ARG((uintptr_t)x % 4 == 0, "corpus_batch: x is not 4-byte aligned");
  VQA_ARG(step >= 0 && corpus_len >= 0, "corpus_batch: negative step or corpus_len");
  return feed_launch<float>("corpus_batch_kernel", pcm == VQA_PCM_I16, B, T, [&](auto s, dim3 grid) {
    hipLaunchKernelGGL(corpus_batch_kernel<decltype(s)>, grid, dim3(256), 0, (hipStream_t)stream,
                       (const decltype(s)*)corpus, (long long)corpus_len, starts, labels, (long long)M, x, labels_out,
                       index_out, B, (long long)T, seed, counter, (long long)step, rank, world, shuffle);
  });
}

extern "C" int vqa_code_batch(const void* codes, int64_t codes_len, const void* upper, int64_t upper_len, int rate,
                              int width, const int64_t* starts, const int64_t* labels, int64_t M, int64_t* z,
                              int64_t* z_upper, int64_t* labels_out, int64_t* index_out, int B, int64_t T,
                              uint64_t seed, const int64_t* counter, int64_t step, int rank, int world, int shuffle,
                              vqa_stream_t stream) {
  VQA_ARG(codes && starts && z, "code_batch: null codes, starts or z");
  if (int rc = feed_args("code_batch", B, T, M, rank, world, labels, labels_out)) return rc;
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
  VQA_ARG(step >= 0 && codes_len >= 0 && upper_len >= 0, "code_batch: negative step, codes_len or upper_len");
  return feed_launch<int32_t>("code_batch_kernel", width == VQA_CODE_I16, B, T, [&](auto s, dim3 grid) {
    hipLaunchKernelGGL(code_batch_kernel<decltype(s)>, grid, dim3(256), 0, (hipStream_t)stream,
                       (const decltype(s)*)codes, (long long)codes_len, (const decltype(s)*)upper,
                       (long long)upper_len, rate, starts, labels, (long long)M, z, z_upper, labels_out, index_out, B,
                       (long long)T, seed, counter, (long long)step, rank, world, shuffle);
  });
}
