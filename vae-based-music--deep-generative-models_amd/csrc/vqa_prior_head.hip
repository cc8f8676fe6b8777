// vqa_prior_head.hip — the prior's output head fused with the cross entropy (gfx950), and the row sums of the
// loss.
//
// Replaces (reference file:line):
//   src/autoregressive/autoregressive_fmha.py:80,158    out = layers.Dense(bins)       -> head_* (fused with the loss)
//   autoregressive.py:189-212, prior.py:272-300          loss / accuracy                -> head_*, rowsum
#include "vqa_prior.h"

namespace vqa {

// ---------------------------------------------------------------------------------------------------
// Output head fused with the loss (autoregressive_fmha.py:80,158 Dense(bins); autoregressive.py:189-212):
// logits = X W + b are never written. Wt = W^T in the activation dtype, (V, 128), prepared once per step.
//   head_fwd:    per row lse, argmax (first maximum, tf.argmax), and with targets the row loss lse - logit[t]
//                and correctness
//   head_bwd_dx: dX = dlogits W^T, dlogits = (softmax - onehot) * inv_count (logits recomputed per vocab tile)
//   head_bwd_dw: dW = X^T dlogits, db = sum dlogits per (vocab tile, row segment) partial
constexpr int HK = 128;            // model width (the head's K)
template <class T> constexpr int hstride() { return HK + 16 / (int)sizeof(T); }

struct HeadArgs {
  const void* x;
  const void* wt;  // (V, HK)
  const float* bias;
  const int64_t* tgt;
  float* lse;
  int64_t* amax;
  float* loss_row;
  float* correct;
  void* dx;
  float* part;  // dW partials: [segment][HK * V + V]
  long long M;
  int V, seg_rows;
  float inv_count;
};

// logits^T of a 16-vocab subtile for one 16-row subtile: lane (row = lane & 15, g) gets vocab 4g .. 4g+3
template <class T>
__device__ __forceinline__ f32x4 head_tile(const T* wtl, const T* xl, int stride) {
  typedef Mfma<T> M;
  const int lane = threadIdx.x & 63, kof = M::koff(lane), col = lane & 15;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kc = 0; kc < HK; kc += M::KS)
    acc = M::mma(M::load(wtl + col * stride + kof + kc), M::load(xl + col * stride + kof + kc), acc);
  return acc;
}

template <class T>
__device__ __forceinline__ void stage_rows128(T* dst, const T* src, long long row0, long long nrows_avail, int nrows) {
  constexpr int VEC = 16 / (int)sizeof(T), CPR = HK / VEC, S = hstride<T>();
  for (int e = threadIdx.x; e < nrows * CPR; e += 256) {
    const int j = e / CPR, q = e - j * CPR;
    uint4 v = {0u, 0u, 0u, 0u};
    if (row0 + j < nrows_avail) v = *(const uint4*)(src + (row0 + j) * HK + q * VEC);
    *(uint4*)(dst + j * S + q * VEC) = v;
  }
}

// 64 rows of HK channels staged HBM -> registers -> LDS: the next tile's loads are issued before the current
// tile's MFMAs, so their latency hides behind them (rows past `avail` are zeros)
template <class T>
struct Rows64Regs {
  static constexpr int VEC = 16 / (int)sizeof(T), CPR = HK / VEC, PER = 64 * CPR / 256, S = hstride<T>();
  uint4 v[PER];
  __device__ __forceinline__ void load(const T* src, long long row0, long long avail) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int e = threadIdx.x + i * 256, j = e / CPR, q = e - j * CPR;
      v[i] = row0 + j < avail ? *(const uint4*)(src + (row0 + j) * HK + q * VEC) : uint4{0u, 0u, 0u, 0u};
    }
  }
  __device__ __forceinline__ void store(T* dst) const {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int e = threadIdx.x + i * 256, j = e / CPR, q = e - j * CPR;
      *(uint4*)(dst + j * S + q * VEC) = v[i];
    }
  }
};

// logits^T of a 16-vocab subtile with the 16 rows' fragments held in registers (xf[kc] = rows' K slice kc)
template <class T>
__device__ __forceinline__ f32x4 head_tile_x(const T* wtl, const typename Mfma<T>::frag (&xf)[HK / Mfma<T>::KS],
                                             int stride) {
  typedef Mfma<T> M;
  const int lane = threadIdx.x & 63, kof = M::koff(lane), col = lane & 15;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kc = 0; kc < HK / M::KS; ++kc) acc = M::mma(M::load(wtl + col * stride + kof + kc * M::KS), xf[kc], acc);
  return acc;
}

// this lane's share of dot(row, w) for a row held as B fragments (xf[kc]: channels kc*KS + koff ..) and a
// (HK) row w of Wt in the activation dtype; grp_sum over the four lane groups completes it
template <class T>
__device__ __forceinline__ float head_dot_row(const typename Mfma<T>::frag (&xf)[HK / Mfma<T>::KS], const T* w) {
  typedef Mfma<T> M;
  const int kof = M::koff(threadIdx.x & 63);
  float acc = 0.f;
#pragma unroll
  for (int kc = 0; kc < HK / M::KS; ++kc) {
    if constexpr (sizeof(T) == 2) {
      const bf16x8 wv = *(const bf16x8*)(w + kc * M::KS + kof);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc = __builtin_fmaf((float)xf[kc][j], (float)wv[j], acc);
    } else {
      acc = __builtin_fmaf(xf[kc], w[kc * M::KS + kof], acc);
    }
  }
  return acc;
}

// the B fragments of a workgroup's rows (wave w: rows 32w + 16s + (lane & 15)) for every K slice
template <class T>
__device__ __forceinline__ void head_xfrags(typename Mfma<T>::frag (&xf)[2][HK / Mfma<T>::KS], const T* X, int stride) {
  typedef Mfma<T> M;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), kof = M::koff(lane), col = lane & 15;
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int kc = 0; kc < HK / M::KS; ++kc) xf[s][kc] = M::load(X + (wave * 32 + s * 16 + col) * stride + kof + kc * M::KS);
}

// workgroup = 128 rows (wave w: rows 32w .. 32w+31 as two 16-row subtiles, their fragments in registers);
// vocab tiles of 64 through LDS, the next one prefetched into registers
template <class T>
__global__ __launch_bounds__(256) void head_fwd_kernel(HeadArgs a) {
  constexpr int S = hstride<T>();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* X = (T*)smem;     // [128][S]
  T* W = X + 128 * S;  // [64][S]
  const long long r0 = (long long)blockIdx.x * 128;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), li = lane & 15, g = lane >> 4;
  stage_rows128<T>(X, (const T*)a.x, r0, a.M, 128);
  Rows64Regs<T> wn;
  wn.load((const T*)a.wt, 0, a.V);
  __syncthreads();
  typename Mfma<T>::frag xf[2][HK / Mfma<T>::KS];
  head_xfrags<T>(xf, X, S);
  long long rows[2];
  int64_t tg[2];
  float m[2], l[2], bv[2], tl[2];
  int bi[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    rows[s] = r0 + wave * 32 + s * 16 + li;
    tg[s] = (a.tgt && rows[s] < a.M) ? a.tgt[rows[s]] : -1;
    m[s] = -INFINITY; l[s] = 0.f; bv[s] = -INFINITY; bi[s] = 0; tl[s] = -INFINITY;
  }
  constexpr float L2E = 1.4426950408889634f;
  // the tile's bias (slots past V: -inf) through LDS, loaded one tile ahead by wave 0 with the weight rows (read
  // straight from global memory after the barrier, each tile waited for its bias loads there)
  __shared__ __attribute__((aligned(16))) float Bt[64];
  float bn = threadIdx.x < 64 && (int)threadIdx.x < a.V ? a.bias[threadIdx.x] : -INFINITY;
  for (int v0 = 0; v0 < a.V; v0 += 64) {
    __syncthreads();
    wn.store(W);
    if (threadIdx.x < 64) Bt[threadIdx.x] = bn;
    if (v0 + 64 < a.V) {
      wn.load((const T*)a.wt, v0 + 64, a.V);
      if (threadIdx.x < 64) bn = v0 + 64 + (int)threadIdx.x < a.V ? a.bias[v0 + 64 + threadIdx.x] : -INFINITY;
    }
    __syncthreads();
    // this lane's 16 vocab slots of the tile: v0 + 16 st + 4 g + i (slots past V: -inf)
    f32x4 bq[4];
#pragma unroll
    for (int st = 0; st < 4; ++st) bq[st] = *(const f32x4*)(Bt + st * 16 + 4 * g);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float x[16];
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const f32x4 acc = head_tile_x<T>(W + st * 16 * S, xf[s], S);
#pragma unroll
        for (int i = 0; i < 4; ++i) x[4 * st + i] = acc[i] + bq[st][i];  // -inf past V
      }
      float mt = x[0];
#pragma unroll
      for (int k = 1; k < 16; ++k) mt = fmaxf(mt, x[k]);
      // the first slot holding the tile maximum (slots ascend in vocab within the lane): tf.argmax's first max
      int ti = 15;
#pragma unroll
      for (int k = 14; k >= 0; --k) ti = x[k] == mt ? k : ti;
      if (mt > bv[s]) {
        bv[s] = mt;
        bi[s] = v0 + (ti >> 2) * 16 + 4 * g + (ti & 3);
      }
      const float mn = fmaxf(m[s], mt);
      if (mn == -INFINITY) continue;  // only vocab slots past V in this lane so far
      const float nm = -mn * L2E;
      float ps = 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k) ps += __builtin_amdgcn_exp2f(__builtin_fmaf(x[k], L2E, nm));
      l[s] = l[s] * __builtin_amdgcn_exp2f((m[s] - mn) * L2E) + ps;
      m[s] = mn;
    }
  }
  // the target's logit, once per row: the row's fragments (registers) . Wt[target] + bias[target]
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const bool tin = tg[s] >= 0 && tg[s] < a.V;
    const float part = tin ? head_dot_row<T>(xf[s], (const T*)a.wt + tg[s] * HK) : 0.f;
    const float dot = grp_sum(part);
    tl[s] = tin ? dot + a.bias[tg[s]] : -INFINITY;
  }
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const float mx = grp_max(m[s]);
    const float lt = grp_sum(l[s] * __expf(m[s] - mx));
    // argmax across the four lane groups: larger value, then the lower index
    // (the two lanes of each pair, in the same order for the values and the indices; the pick is symmetric)
    auto pick = [](float av, int ai, float bv2, int bi2, float& v, int& i) {
      const bool b_wins = bv2 > av || (bv2 == av && bi2 < ai);
      v = b_wins ? bv2 : av;
      i = b_wins ? bi2 : ai;
    };
    {
      float av, bv2;
      int ai, bi2;
      xl::pair16(bv[s], av, bv2);
      xl::pair16(bi[s], ai, bi2);
      pick(av, ai, bv2, bi2, bv[s], bi[s]);
      xl::pair32(bv[s], av, bv2);
      xl::pair32(bi[s], ai, bi2);
      pick(av, ai, bv2, bi2, bv[s], bi[s]);
    }
    const float t = tl[s];
    if (g == 0 && rows[s] < a.M) {
      const float lse = mx + logf(lt);
      a.lse[rows[s]] = lse;
      if (a.amax) a.amax[rows[s]] = bi[s];
      if (a.loss_row) a.loss_row[rows[s]] = lse - t;
      if (a.correct) a.correct[rows[s]] = (int64_t)bi[s] == tg[s] ? 1.f : 0.f;
    }
  }
}

template <class T>
__global__ __launch_bounds__(256) void head_bwd_dx_kernel(HeadArgs a) {
  typedef Att<T> A;
  constexpr int S = hstride<T>();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* X = (T*)smem;
  T* W = X + 128 * S;
  const long long r0 = (long long)blockIdx.x * 128;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), li = lane & 15, g = lane >> 4;
  stage_rows128<T>(X, (const T*)a.x, r0, a.M, 128);
  Rows64Regs<T> wn;
  wn.load((const T*)a.wt, 0, a.V);
  __syncthreads();
  typename Mfma<T>::frag xf[2][HK / Mfma<T>::KS];
  head_xfrags<T>(xf, X, S);
  long long rows[2];
  int64_t tg[2];
  float lse[2];
  f32x4 acc[2][HK / 16];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    rows[s] = r0 + wave * 32 + s * 16 + li;
    const bool in = rows[s] < a.M;
    tg[s] = in ? a.tgt[rows[s]] : -1;
    lse[s] = in ? a.lse[rows[s]] : INFINITY;  // rows past M: softmax 0, no target -> dlogits 0
#pragma unroll
    for (int kt = 0; kt < HK / 16; ++kt) acc[s][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // softmax * inv_count = exp2((z + b) log2e - (lse log2e - log2 inv_count)); the target's -inv_count is added
  // once per row after the loop (dX -= inv_count Wt[target])
  constexpr float L2E = 1.4426950408889634f;
  float nl[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) nl[s] = -(lse[s] * L2E - __log2f(a.inv_count));
  // the tile's bias through LDS, loaded one tile ahead (as head_fwd_kernel)
  __shared__ __attribute__((aligned(16))) float Bt[64];
  float bn = threadIdx.x < 64 && (int)threadIdx.x < a.V ? a.bias[threadIdx.x] : -INFINITY;
  for (int v0 = 0; v0 < a.V; v0 += 64) {
    __syncthreads();
    wn.store(W);
    if (threadIdx.x < 64) Bt[threadIdx.x] = bn;
    if (v0 + 64 < a.V) {
      wn.load((const T*)a.wt, v0 + 64, a.V);
      if (threadIdx.x < 64) bn = v0 + 64 + (int)threadIdx.x < a.V ? a.bias[v0 + 64 + threadIdx.x] : -INFINITY;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float dl[4][4];
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const f32x4 z = head_tile_x<T>(W + st * 16 * S, xf[s], S);
        const f32x4 bq = *(const f32x4*)(Bt + st * 16 + 4 * g);  // slots past V: -inf (probability 0)
#pragma unroll
        for (int i = 0; i < 4; ++i) dl[st][i] = __builtin_amdgcn_exp2f(__builtin_fmaf(z[i] + bq[i], L2E, nl[s]));
      }
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) {
        const float p8[8] = {dl[2 * cc][0], dl[2 * cc][1], dl[2 * cc][2], dl[2 * cc][3],
                             dl[2 * cc + 1][0], dl[2 * cc + 1][1], dl[2 * cc + 1][2], dl[2 * cc + 1][3]};
#pragma unroll
        for (int kt = 0; kt < HK / 16; ++kt) acc[s][kt] = A::mm_rows(W + kt * 16, S, 32 * cc, p8, acc[s][kt]);
      }
      __builtin_amdgcn_sched_barrier(0);  // one row subtile at a time (register pressure)
    }
  }
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    if (rows[s] >= a.M) continue;
    const bool tin = tg[s] >= 0 && tg[s] < a.V;
    const T* wtg = (const T*)a.wt + (tin ? tg[s] : 0) * HK;
#pragma unroll
    for (int kt = 0; kt < HK / 16; ++kt) {
      f32x4 o = acc[s][kt];
      if (tin) o = o - ld4(wtg + kt * 16 + 4 * g) * a.inv_count;  // the one-hot term of dlogits
      st4((T*)a.dx + rows[s] * HK + kt * 16 + 4 * g, o);
    }
  }
}

// workgroup = (vocab tile of 64: wave w owns vocab v0 + 16w .. +15, row segment); logits in the layout
// lane (vocab, g) <- rows 4g .. 4g+3 so that dW = X^T dlogits takes dlogits as the B operand directly
template <class T>
__global__ __launch_bounds__(256) void head_bwd_dw_kernel(HeadArgs a) {
  typedef Mfma<T> M;
  typedef Att<T> A;
  constexpr int S = hstride<T>();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* W = (T*)smem;     // [64][S]
  T* X = W + 64 * S;   // [64][S]
  __shared__ __attribute__((aligned(16))) float Ls[64];  // lse log2e - log2 inv_count (+inf past the segment)
  __shared__ __attribute__((aligned(16))) int Tg[64];     // targets (-1 past the segment)
  const int nvt = (a.V + 63) / 64, vt = blockIdx.x % nvt, seg = blockIdx.x / nvt, v0 = vt * 64;
  const long long rb = (long long)seg * a.seg_rows, re = std::min<long long>(a.M, rb + a.seg_rows);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), li = lane & 15, g = lane >> 4;
  const int v = v0 + wave * 16 + li;
  constexpr float L2E = 1.4426950408889634f;
  const float bl = v < a.V ? a.bias[v] * L2E : -INFINITY;  // vocab slots past V: probability 0
  const float l2inv = __log2f(a.inv_count);
  stage_rows128<T>(W, (const T*)a.wt, v0, a.V, 64);
  f32x4 acc[HK / 16];
#pragma unroll
  for (int kt = 0; kt < HK / 16; ++kt) acc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float db = 0.f;
  const int kof = M::koff(lane);
  // the next row tile (and its lse / targets) prefetched into registers during the current one's MFMAs
  Rows64Regs<T> xn;
  float ln = INFINITY;
  int tn = -1;
  auto fetch = [&](long long c0) {
    xn.load((const T*)a.x, c0, re);
    if (threadIdx.x < 64) {
      const bool in = c0 + threadIdx.x < re;
      ln = in ? a.lse[c0 + threadIdx.x] * L2E - l2inv : INFINITY;
      tn = in ? (int)a.tgt[c0 + threadIdx.x] : -1;
    }
  };
  if (rb < re) fetch(rb);
  __syncthreads();
  typename M::frag wf[HK / M::KS];  // this wave's 16 vocab columns, every K slice
#pragma unroll
  for (int kc = 0; kc < HK / M::KS; ++kc) wf[kc] = M::load(W + (wave * 16 + li) * S + kof + kc * M::KS);
  for (long long c0 = rb; c0 < re; c0 += 64) {
    __syncthreads();
    xn.store(X);
    if (threadIdx.x < 64) {
      Ls[threadIdx.x] = ln;
      Tg[threadIdx.x] = tn;
    }
    if (c0 + 64 < re) fetch(c0 + 64);
    __syncthreads();
    float dl[4][4];
#pragma unroll
    for (int rs = 0; rs < 4; ++rs) {
      // logits[row][v]: A = X rows (rs*16 + col), B = W^T (vocab col)
      f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kc = 0; kc < HK / M::KS; ++kc) z = M::mma(M::load(X + (rs * 16 + li) * S + kof + kc * M::KS), wf[kc], z);
      // rows rs*16 + 4g + i: softmax * inv_count, minus inv_count at the target
      const f32x4 lq = *(const f32x4*)(Ls + rs * 16 + 4 * g);
      const int4 tq = *(const int4*)(Tg + rs * 16 + 4 * g);
      const int tqa[4] = {tq.x, tq.y, tq.z, tq.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float d = __builtin_amdgcn_exp2f(__builtin_fmaf(z[i], L2E, bl - lq[i]));
        if (v == tqa[i]) d -= a.inv_count;
        dl[rs][i] = d;
        db += d;
      }
    }
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      const float p8[8] = {dl[2 * cc][0], dl[2 * cc][1], dl[2 * cc][2], dl[2 * cc][3],
                           dl[2 * cc + 1][0], dl[2 * cc + 1][1], dl[2 * cc + 1][2], dl[2 * cc + 1][3]};
#pragma unroll
      for (int kt = 0; kt < HK / 16; ++kt) acc[kt] = A::mm_rows(X + kt * 16, S, 32 * cc, p8, acc[kt]);
    }
  }
  // partial row of this segment: dW (HK x V, Keras layout) | db (V); lane (vocab col, g) holds k = kt*16+4g+i
  float* part = a.part + (size_t)seg * ((size_t)HK * a.V + a.V);
  if (v < a.V) {
#pragma unroll
    for (int kt = 0; kt < HK / 16; ++kt)
#pragma unroll
      for (int i = 0; i < 4; ++i) part[(size_t)(kt * 16 + 4 * g + i) * a.V + v] = acc[kt][i];
  }
  db = grp_sum(db);
  if (g == 0 && v < a.V) part[(size_t)HK * a.V + v] = db;
}

// W (HK, V) fp32 -> Wt (V, HK) in the activation dtype
template <class T>
__global__ __launch_bounds__(256) void head_wt_kernel(const float* w, T* wt, int V) {
  const long long total = (long long)HK * V;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int k = (int)(e / V), v = (int)(e - (long long)k * V);
    st(wt + (long long)v * HK + k, w[e]);
  }
}

// out[i] = scale * sum_j x[i * n + j]: stage 1 sums fixed chunks of 4096 per workgroup, stage 2 sums the chunk
// results in order (deterministic)
constexpr int kRowsumChunk = 4096;
__global__ __launch_bounds__(256) void rowsum_part_kernel(const float* x, long long n, int nch, float* part) {
  __shared__ float red[4];
  const int row = blockIdx.x / nch, ch = blockIdx.x - row * nch;
  const float* p = x + (long long)row * n;
  const long long j0 = (long long)ch * kRowsumChunk, j1 = std::min<long long>(n, j0 + kRowsumChunk);
  float s = 0.f;
  for (long long j = j0 + threadIdx.x; j < j1; j += 256) s += p[j];
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void rowsum_final_kernel(const float* part, int nch, float scale, float* out) {
  __shared__ float red[4];
  float s = 0.f;
  for (int j = threadIdx.x; j < nch; j += 256) s += part[(long long)blockIdx.x * nch + j];
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = s * scale;
}

// ---------------------------------------------------------------------------------------------------
template <class T>
static int launch_head(int which, const HeadArgs& a, unsigned grid, size_t lds, hipStream_t s) {
  const void* fn = which == 0 ? (const void*)head_fwd_kernel<T>
                              : which == 1 ? (const void*)head_bwd_dx_kernel<T> : (const void*)head_bwd_dw_kernel<T>;
  if (int rc = raise_dyn_lds(fn, lds, "prior")) return rc;
  HeadArgs c = a;
  void* args[] = {&c};
  (void)hipLaunchKernel(fn, dim3(grid), dim3(256), args, lds, s);
  VQA_LAUNCHED("head_kernel");
  return VQA_OK;
}

static int head_segs(int64_t M, int V) {
  const int nvt = (V + 63) / 64;
  const long long want = std::max<long long>(1, (long long)2 * cu_count() / nvt);
  return (int)std::min<long long>(want, (M + 63) / 64);
}

// row segments of head_bwd_dw_kernel: nseg segments of seg_rows rows (a multiple of its 64-row chunk)
static void head_plan(int64_t M, int V, int& nseg, long long& seg_rows) {
  const int segs = head_segs(M, V);
  seg_rows = ((M + segs - 1) / segs + 63) / 64 * 64;
  nseg = (int)((M + seg_rows - 1) / seg_rows);
}

}  // namespace vqa

using namespace vqa;

extern "C" int vqa_head_wt(const float* w, void* wt, int K, int V, int dtype, vqa_stream_t stream) {
  VQA_ARG(w && wt && K == HK && V > 0 && pr_dt(dtype), "head_wt: bad arguments (K must be %d)", HK);
  const unsigned g = pr_grid((long long)K * V);
  if (dtype == VQA_BF16) hipLaunchKernelGGL(head_wt_kernel<bf16>, dim3(g), dim3(256), 0, (hipStream_t)stream, w, (bf16*)wt, V);
  else hipLaunchKernelGGL(head_wt_kernel<float>, dim3(g), dim3(256), 0, (hipStream_t)stream, w, (float*)wt, V);
  VQA_LAUNCHED("head_wt_kernel");
  return VQA_OK;
}

extern "C" int vqa_head_fwd(const void* x, const void* wt, const float* bias, const int64_t* targets, float* lse,
                            int64_t* amax, float* loss_row, float* correct, int64_t M, int K, int V, int dtype,
                            vqa_stream_t stream) {
  VQA_ARG(x && wt && bias && lse && M > 0 && K == HK && V > 0 && pr_dt(dtype), "head_fwd: bad arguments");
  VQA_ARG(!(loss_row || correct) || targets, "head_fwd: loss / correctness need targets");
  HeadArgs a{x, wt, bias, targets, lse, amax, loss_row, correct, nullptr, nullptr, (long long)M, V, 0, 0.f};
  const int esz = dtype == VQA_BF16 ? 2 : 4, S = HK + 16 / esz;
  const size_t lds = (size_t)(128 + 64) * S * esz;
  const unsigned g = (unsigned)((M + 127) / 128);
  hipStream_t s = (hipStream_t)stream;
  return dtype == VQA_BF16 ? launch_head<bf16>(0, a, g, lds, s) : launch_head<float>(0, a, g, lds, s);
}

extern "C" int vqa_head_bwd_plan(int64_t M, int K, int V, int* segs, int64_t* seg_rows) {
  VQA_ARG(segs && seg_rows, "head_bwd_plan: null segs or seg_rows");
  VQA_ARG(M > 0 && K == HK && V > 0, "head_bwd_plan: bad arguments");
  int nseg;
  long long sr;
  head_plan(M, V, nseg, sr);
  *segs = nseg;
  *seg_rows = sr;
  return VQA_OK;
}

extern "C" size_t vqa_head_bwd_workspace(int64_t M, int K, int V) {
  if (M < 1 || K < 1 || V < 1) return 0;
  return (size_t)head_segs(M, V) * ((size_t)K * V + V) * sizeof(float);
}

extern "C" int vqa_head_bwd(const void* x, const void* wt, const float* bias, const int64_t* targets, const float* lse,
                            float inv_count, void* dx, float* dw, float* db, int64_t M, int K, int V, int dtype,
                            void* workspace, size_t ws_bytes, vqa_partials_desc* desc, vqa_stream_t stream) {
  VQA_ARG(x && wt && bias && targets && lse && dx && dw && db && M > 0 && K == HK && V > 0 && pr_dt(dtype),
          "head_bwd: bad arguments");
  const size_t need = vqa_head_bwd_workspace(M, K, V);
  VQA_ARG(workspace && ws_bytes >= need, "head_bwd: workspace %zu < %zu", ws_bytes, need);
  const int nvt = (V + 63) / 64;
  int nseg;
  long long seg_rows;
  head_plan(M, V, nseg, seg_rows);
  HeadArgs a{x, wt, bias, targets, (float*)lse, nullptr, nullptr, nullptr, dx, (float*)workspace, (long long)M, V,
             (int)seg_rows, inv_count};
  const int esz = dtype == VQA_BF16 ? 2 : 4, S = HK + 16 / esz;
  hipStream_t s = (hipStream_t)stream;
  int rc = dtype == VQA_BF16 ? launch_head<bf16>(1, a, (unsigned)((M + 127) / 128), (size_t)(128 + 64) * S * esz, s)
                             : launch_head<float>(1, a, (unsigned)((M + 127) / 128), (size_t)(128 + 64) * S * esz, s);
  if (rc) return rc;
  rc = dtype == VQA_BF16 ? launch_head<bf16>(2, a, (unsigned)(nseg * nvt), (size_t)128 * S * esz, s)
                         : launch_head<float>(2, a, (unsigned)(nseg * nvt), (size_t)128 * S * esz, s);
  if (rc) return rc;
  const vqa_partials_desc d{(const float*)workspace, dw, db, nseg, K * V + V, K * V, 0};
  if (desc) {
    *desc = d;
    return VQA_OK;
  }
  return vqa_reduce_partials(&d, 1, stream);
}

extern "C" size_t vqa_rowsum_workspace(int64_t rows, int64_t n) {
  if (rows < 1 || n < 1) return 0;
  return (size_t)rows * ((n + kRowsumChunk - 1) / kRowsumChunk) * sizeof(float);
}

extern "C" int vqa_rowsum(const float* x, int64_t rows, int64_t n, float scale, float* out, void* workspace,
                          size_t ws_bytes, vqa_stream_t stream) {
  VQA_ARG(x && out && rows > 0 && n > 0 && rows < (1 << 20), "rowsum: bad arguments");
  VQA_ARG(workspace && ws_bytes >= vqa_rowsum_workspace(rows, n), "rowsum: workspace too small");
  const int nch = (int)((n + kRowsumChunk - 1) / kRowsumChunk);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(rowsum_part_kernel, dim3((unsigned)(rows * nch)), dim3(256), 0, s, x, (long long)n, nch,
                     (float*)workspace);
  hipLaunchKernelGGL(rowsum_final_kernel, dim3((unsigned)rows), dim3(256), 0, s, (const float*)workspace, nch, scale,
                     out);
  VQA_LAUNCHED("rowsum_kernel");
  return VQA_OK;
}
