// vqa_optim.hip — the Keras-Adam optimizer of libvqa (gfx950): one launch over the flat fp32 parameter buffer.
//
//   vqa_adam_keras : keras.optimizers.Adam() defaults as applied by TF's ApplyAdam (vqvae.py:144,362).
//   vqa_grad_norm / vqa_adam_keras_clipped : OptimizerV2's clipvalue / clipnorm / global_clipnorm on the stream
//                    (a deterministic norm pass, then the same update on the clipped gradient).
//   vqa_adam_keras_ema / vqa_adam_keras_clipped_ema : the same updates with an exponential moving average of the
//                    weights kept in the same pass; vqa_swap_f32 exchanges the weights and their average.
//   vqa_grad_finite / vqa_adam_keras_guarded / vqa_counter_add_if : a step whose aggregated gradient holds a NaN or
//                    an inf is not applied (Keras' LossScaleOptimizer rule), decided on the device so a captured
//                    step replays the decision.
//   vqa_lr_schedule / vqa_counter_add : a LearningRateSchedule's value at, and the increment of, the device step count.
//
// The five updates are two kernels, one per way of walking memory (adam_stride_kernel, adam_blocks_kernel), each
// with and without the average, behind one host path (launch_adam).
#include "vqa_launch.h"
#include <algorithm>
#include <cmath>

namespace vqa {

// What an update launch works on, built once by the entry point and passed to the kernel by value.
struct AdamArgs {
  float* w;
  const float* g;
  float *m, *v;
  long long n;
  const int64_t* step;
  float lr0;
  const float* lr_dev;  // nullable: a LearningRateSchedule's value at this step (vqa_lr_schedule), instead of lr0
  float b1, b2, eps, gs;
};
// gradient clipping: the variable tables, the modes and their thresholds, the norm pass' results
struct ClipArgs {
  const int64_t* seg_start;
  const int* block_seg;
  int nseg, modes;
  float cv, cn, gcn;  // gcn for the host's checks only: the update reads the factor the norm pass left in stats[2]
  const float *seg_norm, *stats;
};
// the weights' moving average
struct EmaArgs {
  float* ema;
  float decay;
  long long start;
  int dynamic;
};
// the step guard (host only: the kernel takes the two pointers): grad_finite's flag and the skip counters
struct GuardArgs {
  const int* ok;
  int64_t* skips;
};

// TF ApplyAdam (training_ops.cc, non-nesterov): alpha = lr*sqrt(1-b2^t)/(1-b1^t);
// m += (g - m)*(1-b1); v += (g*g - v)*(1-b2); var -= (m*alpha)/(sqrt(v) + eps).
// The step's scalars and the update of one element on the (scaled, clipped) gradient u: the one statement of the
// arithmetic, shared by both Adam kernels below, so w, m and v come out bitwise the same from each of them.
struct AdamStep {
  float alpha, omb1, omb2, eps;
  __device__ __forceinline__ AdamStep(const AdamArgs& a) : eps(a.eps) {
    const float lr = a.lr_dev ? a.lr_dev[0] : a.lr0;
    const float t = (float)(a.step[0] + 1);
    const float b1p = powf(a.b1, t), b2p = powf(a.b2, t);
    alpha = lr * sqrtf(1.f - b2p) / (1.f - b1p);
    omb1 = 1.f - a.b1;
    omb2 = 1.f - a.b2;
  }
  __device__ __forceinline__ void moments(float u, float& mi, float& vi) const {
    mi = mi + (u - mi) * omb1;
    vi = vi + (u * u - vi) * omb2;
  }
  // the new weight from the old one and the moments that moments() left
  __device__ __forceinline__ float weight(float wi, float mi, float vi) const {
    return wi - (mi * alpha) / (sqrtf(vi) + eps);
  }
};

// The moving average of the weights for one launch (tfa MovingAverage's rule, TF's assign_moving_average without
// zero-debias), keyed by the same device step count t = *step as the learning-rate schedule:
//   d = 0 below start_step; min(decay, (1 + n) / (10 + n)), n = t - start_step, when dynamic; decay otherwise
//   a = w_new where d == 0 (a copy: the average is the weights bitwise), else a - (a - w_new) * (1 - d)
// d and 1 - d are formed once, the same for every element and on every rank.
struct EmaStep {
  float omd;
  bool copy;
  __device__ __forceinline__ EmaStep(const int64_t* step, const EmaArgs& e) {
    const long long t = step[0];
    float d = e.decay;
    if (t < e.start) {
      d = 0.f;
    } else if (e.dynamic) {
      const float n = (float)(t - e.start);
      d = fminf(e.decay, (1.f + n) / (10.f + n));
    }
    copy = d == 0.f;
    omd = 1.f - d;
  }
  __device__ __forceinline__ float update(float a, float w_new) const {
    return copy ? w_new : a - (a - w_new) * omd;
  }
};

// The grid-stride walk: every buffer read once, w, m, v (and, with EMA, the weights' moving average) written once.
// The first n4 groups of four go as 16-byte accesses, the elements from 4 * n4 on one by one; both loops stride
// over the grid. n4 = n / 4 when all five buffers are 16-byte aligned; 0 elsewhere and in the plain update, which
// asks no alignment of its buffers: its instance is compiled without the wide loop and keeps the registers of the
// scalar one.
template <bool EMA>
__global__ __launch_bounds__(256) void adam_stride_kernel(AdamArgs a, EmaArgs e, long long n4) {
  if (!EMA) n4 = 0;
  const AdamStep ad(a);
  // Without EMA `av` is dead (the wide loop never runs, every other use is under `if (EMA)`) and the compiler
  // drops it with its load: the plain instance keeps the scalar kernel's 20 VGPRs (profiles/optim_unify.txt).
  const EmaStep av(a.step, e);
  float *w = a.w, *m = a.m, *v = a.v, *ema = e.ema;
  const float* g = a.g;
  const long long first = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = first; i < n4; i += stride) {
    const f32x4 gq = ((const f32x4*)g)[i];
    f32x4 mq = ((const f32x4*)m)[i], vq = ((const f32x4*)v)[i], wq = ((const f32x4*)w)[i], aq = ((const f32x4*)ema)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float mi = mq[k], vi = vq[k];
      ad.moments(gq[k] * a.gs, mi, vi);
      mq[k] = mi;
      vq[k] = vi;
      wq[k] = ad.weight(wq[k], mi, vi);
      aq[k] = av.update(aq[k], wq[k]);
    }
    ((f32x4*)m)[i] = mq;
    ((f32x4*)v)[i] = vq;
    ((f32x4*)w)[i] = wq;
    ((f32x4*)ema)[i] = aq;
  }
  for (long long i = 4 * n4 + first; i < a.n; i += stride) {
    float mi = m[i], vi = v[i];
    ad.moments(g[i] * a.gs, mi, vi);
    const float wi = ad.weight(w[i], mi, vi), ai = EMA ? av.update(ema[i], wi) : 0.f;
    m[i] = mi;
    v[i] = vi;
    w[i] = wi;
    if (EMA) ema[i] = ai;
  }
}

// a <-> b, element by element: exact, no temporary buffer. 16-byte accesses for the first n4 groups of four
// (n4 = n / 4 when both buffers are 16-byte aligned, else 0), then one by one.
__global__ __launch_bounds__(256) void swap_kernel(float* a, float* b, long long n, long long n4) {
  const long long first = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = first; i < n4; i += stride) {
    const f32x4 x = ((const f32x4*)a)[i], y = ((const f32x4*)b)[i];
    ((f32x4*)a)[i] = y;
    ((f32x4*)b)[i] = x;
  }
  for (long long i = 4 * n4 + first; i < n; i += stride) {
    const float x = a[i], y = b[i];
    a[i] = y;
    b[i] = x;
  }
}

// ---- gradient clipping (keras OptimizerV2 clipvalue / clipnorm / global_clipnorm) --------------------------
// The flat buffers are cut into blocks of VQA_CLIP_BLOCK floats, one workgroup each, in the norm pass and in the
// block walk of the update alike. A variable is [seg_start[s], seg_start[s + 1]) (the last one ends at n; the
// alignment gap behind a variable is zero in the gradient and counts with it); block_seg[b] is the variable that
// holds the block's first element. Both tables come from the caller; the kernels clamp what they read from them,
// so a wrong table gives wrong sums, never an access outside the buffers.
constexpr int kClipBlock = VQA_CLIP_BLOCK;
static_assert(kClipBlock == 256 * 16, "four float4 per thread and block");

// u = grad_scale * g, then the clipvalue clamp by comparisons (a NaN stays a NaN, as under tf.minimum / tf.maximum)
__device__ __forceinline__ float clip_clamp(float u, float c) {
  u = u < -c ? -c : u;
  return u > c ? c : u;
}

__device__ __forceinline__ int clip_block_seg(const int* block_seg, int nseg) {
  const int s = block_seg[blockIdx.x];
  return s < 0 ? 0 : (s >= nseg ? nseg - 1 : s);
}

// sum over 256 threads of an unsigned count (integer adds: any order gives the same bits)
__device__ __forceinline__ unsigned block_count_256(unsigned c, unsigned* slot) {
  __syncthreads();
  if (threadIdx.x == 0) *slot = 0u;
  __syncthreads();
  if (c) atomicAdd(slot, c);
  __syncthreads();
  return *slot;
}

// Stage 1: block b reads its elements once. Each piece (the part of variable s inside block b) gets the slot b + s of `part`
// (3 words: sum u^2 before the clamp, after it, clamped elements); b + s grows from one piece to the next, so the
// slots are distinct, and there are fewer than blocks + nseg of them. Per thread the squares are added in address
// order, then wave and block trees: the order depends on the layout only.
__global__ __launch_bounds__(256) void grad_norm_pieces_kernel(const float* g, long long n, const int64_t* seg_start,
                                                              const int* block_seg, int nseg, float gs, int clamp,
                                                              float cv, float* part) {
  __shared__ float red[4];
  __shared__ unsigned cnt_slot;
  const long long b0 = (long long)blockIdx.x * kClipBlock;
  const long long b1 = b0 + kClipBlock < n ? b0 + kClipBlock : n;
  int s = clip_block_seg(block_seg, nseg);
  long long p0 = b0;
  for (;;) {
    long long p1 = b1;
    if (s + 1 < nseg) {
      const long long nx = seg_start[s + 1] & ~3LL;
      p1 = nx < p0 ? p0 : (nx < b1 ? nx : b1);
    }
    float raw = 0.f, cl = 0.f;
    unsigned cnt = 0u;
    const long long len4 = (p1 - p0) >> 2;
    for (long long i = threadIdx.x; i < len4; i += 256) {
      const f32x4 q = ((const f32x4*)(g + p0))[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float u = q[k] * gs;
        raw += u * u;
        if (clamp) {
          const float c = clip_clamp(u, cv);
          cnt += (u < -cv || u > cv) ? 1u : 0u;
          cl += c * c;
        }
      }
    }
    if (threadIdx.x == 0) {  // the buffer's last one to three elements
      for (long long i = p0 + 4 * len4; i < p1; ++i) {
        const float u = g[i] * gs;
        raw += u * u;
        if (clamp) {
          const float c = clip_clamp(u, cv);
          cnt += (u < -cv || u > cv) ? 1u : 0u;
          cl += c * c;
        }
      }
    }
    raw = block_sum_256(raw, red);
    if (clamp) {
      cl = block_sum_256(cl, red);
      cnt = block_count_256(cnt, &cnt_slot);
    } else {
      cl = raw;
    }
    if (threadIdx.x == 0) {
      float* o = part + 3 * ((long long)blockIdx.x + s);
      o[0] = raw;
      o[1] = cl;
      ((unsigned*)o)[2] = cnt;
    }
    if (p1 >= b1) break;
    p0 = p1;
    ++s;
  }
}

// Stage 2: one wave per variable adds the variable's pieces, lane l taking pieces l, l + 64, ... in order, then
// the wave tree. seg_norm = sqrt(s2) where s2 > 0, s2 itself elsewhere (tf.clip_by_norm: 0, or a NaN kept).
__global__ __launch_bounds__(256) void grad_norm_segments_kernel(const float* part, long long n,
                                                                const int64_t* seg_start, int nseg, float* seg_raw,
                                                                float* seg_s2, unsigned* seg_cnt, float* seg_norm) {
  __shared__ unsigned cnt_slot[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = blockIdx.x * 4 + wave;
  if (lane == 0) cnt_slot[wave] = 0u;
  __syncthreads();
  float raw = 0.f, cl = 0.f;
  unsigned cnt = 0u;
  if (s < nseg) {
    long long a = seg_start[s], e = s + 1 < nseg ? seg_start[s + 1] : n;
    a = a < 0 ? 0 : (a > n ? n : a);
    e = e < a ? a : (e > n ? n : e);
    if (e > a) {
      const long long bl = (e - 1) / kClipBlock;
      for (long long b = a / kClipBlock + lane; b <= bl; b += 64) {
        const float* o = part + 3 * (b + s);
        raw += o[0];
        cl += o[1];
        cnt += ((const unsigned*)o)[2];
      }
    }
  }
  raw = warp_sum(raw);
  cl = warp_sum(cl);
  if (cnt) atomicAdd(&cnt_slot[wave], cnt);
  __syncthreads();
  if (s < nseg && lane == 0) {
    seg_raw[s] = raw;
    seg_s2[s] = cl;
    seg_cnt[s] = cnt_slot[wave];
    seg_norm[s] = cl > 0.f ? sqrtf(cl) : cl;
  }
}

// Stage 3: one workgroup adds the variables (thread t takes t, t + 256, ... in order, then the block tree) and
// writes the statistics: [0] |u| before any clipping, [1] |u| after clipvalue (what the norm modes see),
// [2] the factor global_clipnorm applies (tf.clip_by_global_norm: c * min(1/norm, 1/c), NaN for a non-finite norm;
// 1 when off), [3] variables whose norm exceeds clipnorm (0 when off), [4] elements clipvalue clamped, [5..7] 0.
__global__ __launch_bounds__(256) void grad_norm_stats_kernel(const float* seg_raw, const float* seg_s2,
                                                             const unsigned* seg_cnt, const float* seg_norm, int nseg,
                                                             int modes, float cn, float gcn, float* stats) {
  __shared__ float red[4];
  __shared__ unsigned cnt_slot;
  float raw = 0.f, cl = 0.f;
  unsigned cnt = 0u, over = 0u;
  for (int s = threadIdx.x; s < nseg; s += 256) {
    raw += seg_raw[s];
    cl += seg_s2[s];
    cnt += seg_cnt[s];
    if ((modes & VQA_CLIP_NORM) && seg_norm[s] > cn) ++over;
  }
  raw = block_sum_256(raw, red);
  cl = block_sum_256(cl, red);
  cnt = block_count_256(cnt, &cnt_slot);
  over = block_count_256(over, &cnt_slot);
  if (threadIdx.x != 0) return;
  const float norm = sqrtf(cl);
  float scale = 1.f;
  if (modes & VQA_CLIP_GLOBAL_NORM) {
    const float a = 1.f / norm, b = 1.f / gcn;
    scale = isfinite(norm) ? gcn * (a < b ? a : b) : __builtin_nanf("");
  }
  stats[0] = sqrtf(raw);
  stats[1] = norm;
  stats[2] = scale;
  stats[3] = (float)over;
  stats[4] = (float)cnt;
  stats[5] = stats[6] = stats[7] = 0.f;
}

// ---- skipping non-finite steps ---------------------------------------------------------------------------
// ok[0] = 1 iff every float of g is finite (the exponent field is not all ones: any finite value, denormals and
// -0.0 pass; NaN and +-inf do not). flag_set_kernel writes the 1, grad_finite_kernel clears it with an integer
// atomic AND: nothing is kept between calls and the result does not depend on the order of the workgroups.
// One grid-stride loop over units: first the n4 groups of four behind the `head` floats that precede the first
// 16-byte boundary (16-byte loads), then those head floats and the tail behind the last whole group one by one.
__global__ void flag_set_kernel(int* ok) {
  if (threadIdx.x == 0 && blockIdx.x == 0) ok[0] = 1;
}

__device__ __forceinline__ bool finite_f32(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(256) void grad_finite_kernel(const float* g, long long n, long long head, long long n4,
                                                         int* ok) {
  const long long tail0 = head + 4 * n4;           // the first element behind the groups of four
  const long long units = n4 + head + (n - tail0);  // groups, then the head's and the tail's single floats
  const f32x4* q = (const f32x4*)(g + head);
  bool fin = true;
  for (long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x; u < units;
       u += (long long)gridDim.x * blockDim.x) {
    if (u < n4) {
      const f32x4 x = q[u];
      fin = fin && finite_f32(x[0]) && finite_f32(x[1]) && finite_f32(x[2]) && finite_f32(x[3]);
    } else {
      const long long j = u - n4;
      fin = fin && finite_f32(g[j < head ? j : tail0 + (j - head)]);
    }
  }
  if (__any(!fin) && (threadIdx.x & 63) == 0) atomicAnd(ok, 0);
}

// The guard of one update launch: is the step applied (ok[0] == 1)? The launch's first thread keeps the counters,
// skips[0] = steps skipped in all, skips[1] = steps skipped in a row. No other thread touches them.
__device__ __forceinline__ bool guard_step(const int* ok, int64_t* skips) {
  const bool go = ok[0] == 1;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (go) {
      skips[1] = 0;
    } else {
      skips[0] += 1;
      skips[1] += 1;
    }
  }
  return go;
}

// The block walk, one block of VQA_CLIP_BLOCK floats per workgroup: the update on u = clip(grad_scale * g):
// clipvalue, then clipnorm ((u * c) / max(norm, c), the NaN of a norm kept), then global_clipnorm (u * stats[2]) —
// OptimizerV2._transform_gradients' order. With modes == 0 that is the plain update, u = grad_scale * g, and
// nothing of `c` is read. g is only read. A float4 never straddles two variables (offsets are multiples of 4), so
// a thread finds its variable once per float4, walking forward from the block's first one.
// EMA: the weights' moving average (EmaStep) goes with them, ema read and written like w.
// ok (nullable): the flag of a guarded step, skips its counters (guard_step); a skipped step returns before any
// load or store of w, m, v and ema. With a null ok the update is unconditional and skips is not touched.
template <bool EMA>
__global__ __launch_bounds__(256) void adam_blocks_kernel(AdamArgs a, ClipArgs c, EmaArgs e, const int* ok,
                                                         int64_t* skips) {
  if (ok && !guard_step(ok, skips)) return;
  const AdamStep ad(a);
  const EmaStep av(a.step, e);  // dead without EMA (every use is under `if (EMA)`): the compiler drops it
  float *w = a.w, *m = a.m, *v = a.v, *ema = e.ema;
  const float* g = a.g;
  const long long n = a.n;
  const float gscale = (c.modes & VQA_CLIP_GLOBAL_NORM) ? c.stats[2] : 1.f;
  const long long b0 = (long long)blockIdx.x * kClipBlock;
  int s = 0;
  long long next = 0x7fffffffffffffffLL;
  if (c.modes & VQA_CLIP_NORM) {
    s = clip_block_seg(c.block_seg, c.nseg);
    if (s + 1 < c.nseg) next = c.seg_start[s + 1];
  }
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const long long p = b0 + 4LL * (it * 256 + (int)threadIdx.x);
    if (p >= n) break;
    float den = 1.f;
    if (c.modes & VQA_CLIP_NORM) {
      while (next <= p) {
        ++s;
        next = s + 1 < c.nseg ? c.seg_start[s + 1] : 0x7fffffffffffffffLL;
      }
      const float nm = c.seg_norm[s];
      den = nm < c.cn ? c.cn : nm;  // max(norm, c); a NaN norm compares false and stays
    }
    const int cnt = n - p >= 4 ? 4 : (int)(n - p);
    f32x4 gq, mq, vq, wq, aq = {0.f, 0.f, 0.f, 0.f};
    if (cnt == 4) {
      gq = *(const f32x4*)(g + p);
      mq = *(const f32x4*)(m + p);
      vq = *(const f32x4*)(v + p);
      wq = *(const f32x4*)(w + p);
      if (EMA) aq = *(const f32x4*)(ema + p);
    } else {
      for (int k = 0; k < 4; ++k) {
        const bool in = k < cnt;
        gq[k] = in ? g[p + k] : 0.f;
        mq[k] = in ? m[p + k] : 0.f;
        vq[k] = in ? v[p + k] : 0.f;
        wq[k] = in ? w[p + k] : 0.f;
        if (EMA) aq[k] = in ? ema[p + k] : 0.f;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float u = gq[k] * a.gs;
      if (c.modes & VQA_CLIP_VALUE) u = clip_clamp(u, c.cv);
      if (c.modes & VQA_CLIP_NORM) u = (u * c.cn) / den;
      if (c.modes & VQA_CLIP_GLOBAL_NORM) u = u * gscale;
      float mi = mq[k], vi = vq[k];
      ad.moments(u, mi, vi);
      mq[k] = mi;
      vq[k] = vi;
      wq[k] = ad.weight(wq[k], mi, vi);
      if (EMA) aq[k] = av.update(aq[k], wq[k]);
    }
    if (cnt == 4) {
      *(f32x4*)(m + p) = mq;
      *(f32x4*)(v + p) = vq;
      *(f32x4*)(w + p) = wq;
      if (EMA) *(f32x4*)(ema + p) = aq;
    } else {
      for (int k = 0; k < cnt; ++k) {
        m[p + k] = mq[k];
        v[p + k] = vq[k];
        w[p + k] = wq[k];
        if (EMA) ema[p + k] = aq[k];
      }
    }
  }
}

// keras LearningRateSchedule evaluated on the device at the optimizer's step counter (OptimizerV2._decayed_lr
// calls the schedule with float(iterations), the count BEFORE this step's increment), so a captured step replays
// with the right rate. Host-precomputed float32 constants keep the arithmetic TF's:
//   kind 1  CustomSchedule (src/transformer/multi_head_attention.py:82-101): p0 = rsqrt(d_model),
//           p1 = warmup_steps ** -1.5 -> p0 * min(rsqrt(s), s * p1)
//   kind 2  keras ExponentialDecay: p0 = initial rate, p1 = decay_steps, p2 = decay_rate, p3 = staircase (0 / 1)
//           -> p0 * p2 ** (s / p1), the exponent floored when staircase
__global__ void lr_schedule_kernel(const int64_t* step, float* lr, int kind, float p0, float p1, float p2, float p3) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float s = (float)step[0];
  float r = p0;
  if (kind == 1) {
    r = p0 * fminf(1.0f / sqrtf(s), s * p1);
  } else if (kind == 2) {
    float e = s / p1;
    if (p3 != 0.f) e = floorf(e);
    r = p0 * powf(p2, e);
  }
  lr[0] = r;
}

// ok (nullable): the flag of a guarded step, whose step counter advances only when the step was applied
__global__ void counter_add_kernel(int64_t* c, int64_t delta, const int* ok) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (ok && ok[0] != 1) return;
  c[0] += delta;
}

// ---- host: argument checks shared by the entry points
static bool overlap(const float* a, const float* b, int64_t n) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, bytes = (uintptr_t)n * sizeof(float);
  return x < y ? y - x < bytes : x - y < bytes;
}

// do the 8 bytes at `a` and the `nb` int64 at `b` share a byte?
static bool overlap_i64(const int64_t* a, const int64_t* b, int nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y ? y - x < sizeof(int64_t) : x - y < (uintptr_t)nb * sizeof(int64_t);
}

static int ema_check(const char* what, const float* w, int64_t n, const EmaArgs& e) {
  VQA_ARG(n > 0, "%s: n must be > 0 (got %lld)", what, (long long)n);
  VQA_ARG(e.ema, "%s: null average", what);
  VQA_ARG(!w || !overlap(w, e.ema, n), "%s: the average must not alias the weights", what);
  VQA_ARG(std::isfinite(e.decay) && e.decay >= 0.f && e.decay < 1.f,
          "%s: average_decay must be finite and in [0, 1) (got %g)", what, (double)e.decay);
  VQA_ARG(e.start >= 0, "%s: start_step must be >= 0 (got %lld)", what, e.start);
  VQA_ARG(e.dynamic == 0 || e.dynamic == 1, "%s: dynamic must be 0 or 1 (got %d)", what, e.dynamic);
  return VQA_OK;
}

static long long clip_blocks(int64_t n) { return (n + kClipBlock - 1) / kClipBlock; }

static bool clip_threshold_ok(int modes, int bit, float c) { return !(modes & bit) || (std::isfinite(c) && c > 0.f); }

static int clip_check(const char* what, int64_t n, const ClipArgs& c) {
  VQA_ARG(n > 0, "%s: n must be > 0 (got %lld)", what, (long long)n);
  VQA_ARG(c.nseg > 0, "%s: nseg must be > 0 (got %d)", what, c.nseg);
  VQA_ARG(clip_blocks(n) + c.nseg < (1LL << 31), "%s: n %lld too large", what, (long long)n);
  VQA_ARG(c.seg_start && c.block_seg, "%s: null variable table", what);
  VQA_ARG((c.modes & ~(VQA_CLIP_VALUE | VQA_CLIP_NORM | VQA_CLIP_GLOBAL_NORM)) == 0, "%s: unknown mode bits %d", what,
          c.modes);
  VQA_ARG(!((c.modes & VQA_CLIP_NORM) && (c.modes & VQA_CLIP_GLOBAL_NORM)),
          "%s: clipnorm and global_clipnorm exclude each other", what);
  VQA_ARG(clip_threshold_ok(c.modes, VQA_CLIP_VALUE, c.cv), "%s: clipvalue must be finite and > 0 (got %g)", what,
          (double)c.cv);
  VQA_ARG(clip_threshold_ok(c.modes, VQA_CLIP_NORM, c.cn), "%s: clipnorm must be finite and > 0 (got %g)", what,
          (double)c.cn);
  VQA_ARG(clip_threshold_ok(c.modes, VQA_CLIP_GLOBAL_NORM, c.gcn), "%s: global_clipnorm must be finite and > 0 (got %g)",
          what, (double)c.gcn);
  return VQA_OK;
}

// The one host path of the five updates. `what` is the entry point's name in its messages; clip, ema and guard are
// null where the entry point has no such part (vqa_adam_keras_guarded: no clip with modes == 0, no ema with a null
// average). A clipped or guarded update takes the block walk and demands 16-byte alignment; the plain and the
// averaging update stride over the grid and take any 4-byte aligned buffers.
static int launch_adam(const char* what, const AdamArgs& a, const ClipArgs* clip, const EmaArgs* ema,
                       const GuardArgs* guard, vqa_stream_t stream) {
  if (guard) {
    VQA_ARG(a.n > 0, "%s: n must be > 0 (got %lld)", what, a.n);
    VQA_ARG(guard->ok, "%s: null ok flag", what);
    VQA_ARG(guard->skips, "%s: null skip counters", what);
    VQA_ARG(!a.step || !overlap_i64(a.step, guard->skips, 2), "%s: the skip counters must not alias the step counter",
            what);
  }
  int rc = VQA_OK;
  if (clip) {
    rc = clip_check(what, a.n, *clip);
    if (rc != VQA_OK) return rc;
    if (guard) VQA_ARG(clip->seg_norm && clip->stats, "%s: null pointer (seg_norm, stats)", what);
  } else if (guard) {
    VQA_ARG(clip_blocks(a.n) < (1LL << 31), "%s: n %lld too large", what, a.n);
  }
  if (ema) {
    rc = ema_check(what, a.w, a.n, *ema);
    if (rc != VQA_OK) return rc;
  }
  VQA_ARG(a.n > 0 && a.w && a.g && a.m && a.v && a.step && (!clip || (clip->seg_norm && clip->stats)), "%s: %s", what,
          clip || ema || guard ? "null pointer" : "bad arguments");
  const EmaArgs e = ema ? *ema : EmaArgs{};
  const bool aligned = ((uintptr_t)a.w | (uintptr_t)a.g | (uintptr_t)a.m | (uintptr_t)a.v | (uintptr_t)e.ema) % 16 == 0;
  hipStream_t s = (hipStream_t)stream;
  if (!clip && !guard) {
    const bool wide = ema && aligned;
    const long long n4 = wide ? a.n / 4 : 0;
    const dim3 grid(blocks_for(wide ? n4 : a.n, 4096));
    if (ema)
      hipLaunchKernelGGL(adam_stride_kernel<true>, grid, dim3(256), 0, s, a, e, n4);
    else
      hipLaunchKernelGGL(adam_stride_kernel<false>, grid, dim3(256), 0, s, a, e, n4);
    VQA_LAUNCHED("adam_stride_kernel");
    return VQA_OK;
  }
  VQA_ARG(aligned, "%s: %s must be 16-byte aligned", what,
          guard ? "w, g, m, v and the average" : ema ? "w, g, m, v and ema" : "w, g, m and v");
  const ClipArgs c = clip ? *clip : ClipArgs{};
  const GuardArgs gd = guard ? *guard : GuardArgs{};
  const dim3 grid((int)clip_blocks(a.n));
  if (ema)
    hipLaunchKernelGGL(adam_blocks_kernel<true>, grid, dim3(256), 0, s, a, c, e, gd.ok, gd.skips);
  else
    hipLaunchKernelGGL(adam_blocks_kernel<false>, grid, dim3(256), 0, s, a, c, e, gd.ok, gd.skips);
  VQA_LAUNCHED("adam_blocks_kernel");
  return VQA_OK;
}

}  // namespace vqa

using namespace vqa;

extern "C" int vqa_adam_keras(float* w, const float* g, float* m, float* v, int64_t n, const int64_t* step, float lr,
                              const float* lr_dev, float beta1, float beta2, float eps, float grad_scale,
                              vqa_stream_t stream) {
  const AdamArgs a{w, g, m, v, (long long)n, step, lr, lr_dev, beta1, beta2, eps, grad_scale};
  return launch_adam("adam", a, nullptr, nullptr, nullptr, stream);
}

extern "C" int vqa_adam_keras_ema(float* w, const float* g, float* m, float* v, int64_t n, const int64_t* step,
                                  float lr, const float* lr_dev, float beta1, float beta2, float eps,
                                  float grad_scale, float* ema, float average_decay, int64_t start_step, int dynamic,
                                  vqa_stream_t stream) {
  const AdamArgs a{w, g, m, v, (long long)n, step, lr, lr_dev, beta1, beta2, eps, grad_scale};
  const EmaArgs e{ema, average_decay, (long long)start_step, dynamic};
  return launch_adam("adam_ema", a, nullptr, &e, nullptr, stream);
}

extern "C" int vqa_swap_f32(float* a, float* b, int64_t n, vqa_stream_t stream) {
  VQA_ARG(n > 0, "swap: n must be > 0 (got %lld)", (long long)n);
  VQA_ARG(a && b, "swap: null pointer");
  VQA_ARG(a != b && !overlap(a, b, n), "swap: the two buffers must not be the same or overlap");
  const bool wide = ((uintptr_t)a | (uintptr_t)b) % 16 == 0;
  const long long n4 = wide ? n / 4 : 0;
  hipLaunchKernelGGL(swap_kernel, dim3(blocks_for(wide ? n4 : n, 4096)), dim3(256), 0, (hipStream_t)stream, a, b,
                     (long long)n, n4);
  VQA_LAUNCHED("swap_kernel");
  return VQA_OK;
}

// 3 words per piece slot (blocks + nseg slots), then per variable: sum u^2 before the clamp, after it, clamped count
extern "C" size_t vqa_grad_norm_workspace(int64_t n, int nseg) {
  if (n < 1 || nseg < 1) return 0;
  return (size_t)(3 * (clip_blocks(n) + nseg) + 3 * (long long)nseg) * sizeof(float);
}

extern "C" int vqa_grad_norm(const float* g, int64_t n, const int64_t* seg_start, const int32_t* block_seg, int nseg,
                             float grad_scale, int modes, float clipvalue, float clipnorm, float global_clipnorm,
                             float* seg_norm, float* stats, void* workspace, size_t ws_bytes, vqa_stream_t stream) {
  const ClipArgs c{seg_start, block_seg, nseg, modes, clipvalue, clipnorm, global_clipnorm, seg_norm, stats};
  const int rc = clip_check("grad_norm", n, c);
  if (rc != VQA_OK) return rc;
  VQA_ARG(g && seg_norm && stats, "grad_norm: null pointer");
  VQA_ARG((uintptr_t)g % 16 == 0, "grad_norm: the gradient must be 16-byte aligned");
  VQA_ARG(workspace && ws_bytes >= vqa_grad_norm_workspace(n, nseg), "grad_norm: workspace too small (%zu B, need %zu)",
          ws_bytes, vqa_grad_norm_workspace(n, nseg));
  hipStream_t s = (hipStream_t)stream;
  const int nb = (int)clip_blocks(n);
  float* part = (float*)workspace;
  float* seg_raw = part + 3 * ((long long)nb + nseg);
  float* seg_s2 = seg_raw + nseg;
  unsigned* seg_cnt = (unsigned*)(seg_s2 + nseg);
  hipLaunchKernelGGL(grad_norm_pieces_kernel, dim3(nb), dim3(256), 0, s, g, (long long)n, seg_start, block_seg, nseg,
                     grad_scale, (modes & VQA_CLIP_VALUE) ? 1 : 0, clipvalue, part);
  VQA_LAUNCHED("grad_norm_pieces_kernel");
  hipLaunchKernelGGL(grad_norm_segments_kernel, dim3((nseg + 3) / 4), dim3(256), 0, s, (const float*)part, (long long)n,
                     seg_start, nseg, seg_raw, seg_s2, seg_cnt, seg_norm);
  VQA_LAUNCHED("grad_norm_segments_kernel");
  hipLaunchKernelGGL(grad_norm_stats_kernel, dim3(1), dim3(256), 0, s, (const float*)seg_raw, (const float*)seg_s2,
                     (const unsigned*)seg_cnt, (const float*)seg_norm, nseg, modes, clipnorm, global_clipnorm, stats);
  VQA_LAUNCHED("grad_norm_stats_kernel");
  return VQA_OK;
}

extern "C" int vqa_adam_keras_clipped(float* w, const float* g, float* m, float* v, int64_t n, const int64_t* step,
                                      float lr, const float* lr_dev, float beta1, float beta2, float eps,
                                      float grad_scale, const int64_t* seg_start, const int32_t* block_seg, int nseg,
                                      int modes, float clipvalue, float clipnorm, float global_clipnorm,
                                      const float* seg_norm, const float* stats, vqa_stream_t stream) {
  const AdamArgs a{w, g, m, v, (long long)n, step, lr, lr_dev, beta1, beta2, eps, grad_scale};
  const ClipArgs c{seg_start, block_seg, nseg, modes, clipvalue, clipnorm, global_clipnorm, seg_norm, stats};
  return launch_adam("adam_clipped", a, &c, nullptr, nullptr, stream);
}

extern "C" int vqa_adam_keras_clipped_ema(float* w, const float* g, float* m, float* v, int64_t n, const int64_t* step,
                                          float lr, const float* lr_dev, float beta1, float beta2, float eps,
                                          float grad_scale, const int64_t* seg_start, const int32_t* block_seg,
                                          int nseg, int modes, float clipvalue, float clipnorm, float global_clipnorm,
                                          const float* seg_norm, const float* stats, float* ema, float average_decay,
                                          int64_t start_step, int dynamic, vqa_stream_t stream) {
  const AdamArgs a{w, g, m, v, (long long)n, step, lr, lr_dev, beta1, beta2, eps, grad_scale};
  const ClipArgs c{seg_start, block_seg, nseg, modes, clipvalue, clipnorm, global_clipnorm, seg_norm, stats};
  const EmaArgs e{ema, average_decay, (long long)start_step, dynamic};
  return launch_adam("adam_clipped_ema", a, &c, &e, nullptr, stream);
}

extern "C" int vqa_grad_finite(const float* g, int64_t n, int32_t* ok, vqa_stream_t stream) {
  VQA_ARG(n > 0, "grad_finite: n must be > 0 (got %lld)", (long long)n);
  VQA_ARG(g && ok, "grad_finite: null pointer");
  VQA_ARG((uintptr_t)g % 4 == 0 && (uintptr_t)ok % 4 == 0, "grad_finite: g and ok must be 4-byte aligned");
  const long long head = std::min<long long>((long long)((16 - (uintptr_t)g % 16) % 16 / 4), n);
  const long long n4 = (n - head) / 4, units = n4 + (n - 4 * n4);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(flag_set_kernel, dim3(1), dim3(64), 0, s, ok);
  VQA_LAUNCHED("flag_set_kernel");
  hipLaunchKernelGGL(grad_finite_kernel, dim3(blocks_for(units, VQA_FINITE_MAX_BLOCKS)), dim3(256), 0, s, g,
                     (long long)n, head, n4, ok);
  VQA_LAUNCHED("grad_finite_kernel");
  return VQA_OK;
}

// the plain form (modes == 0) reads no table; without an average (ema null) its settings are ignored
extern "C" int vqa_adam_keras_guarded(float* w, const float* g, float* m, float* v, int64_t n, const int64_t* step,
                                      float lr, const float* lr_dev, float beta1, float beta2, float eps,
                                      float grad_scale, const int64_t* seg_start, const int32_t* block_seg, int nseg,
                                      int modes, float clipvalue, float clipnorm, float global_clipnorm,
                                      const float* seg_norm, const float* stats, float* ema, float average_decay,
                                      int64_t start_step, int dynamic, const int32_t* ok, int64_t* skip_counters,
                                      vqa_stream_t stream) {
  const AdamArgs a{w, g, m, v, (long long)n, step, lr, lr_dev, beta1, beta2, eps, grad_scale};
  const ClipArgs c{seg_start, block_seg, nseg, modes, clipvalue, clipnorm, global_clipnorm, seg_norm, stats};
  const EmaArgs e{ema, average_decay, (long long)start_step, dynamic};
  const GuardArgs gd{ok, skip_counters};
  return launch_adam("adam_guarded", a, modes ? &c : nullptr, ema ? &e : nullptr, &gd, stream);
}

extern "C" int vqa_lr_schedule(const int64_t* step, float* lr, int kind, float p0, float p1, float p2, float p3,
                               vqa_stream_t stream) {
  VQA_ARG(step && lr && kind >= 0 && kind <= 2, "lr_schedule: bad arguments (kind %d)", kind);
  VQA_ARG(kind != 2 || p1 > 0.f, "lr_schedule: decay_steps must be > 0");
  hipLaunchKernelGGL(lr_schedule_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, step, lr, kind, p0, p1, p2, p3);
  VQA_LAUNCHED("lr_schedule_kernel");
  return VQA_OK;
}

extern "C" int vqa_counter_add(int64_t* counter, int64_t delta, vqa_stream_t stream) {
  VQA_ARG(counter, "counter_add: null pointer");
  hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, counter, delta,
                     (const int*)nullptr);
  VQA_LAUNCHED("counter_add_kernel");
  return VQA_OK;
}

extern "C" int vqa_counter_add_if(int64_t* counter, int64_t delta, const int32_t* ok, vqa_stream_t stream) {
  VQA_ARG(counter, "counter_add_if: null pointer");
  VQA_ARG(ok, "counter_add_if: null ok flag");
  hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, counter, delta, ok);
  VQA_LAUNCHED("counter_add_kernel");
  return VQA_OK;
}
