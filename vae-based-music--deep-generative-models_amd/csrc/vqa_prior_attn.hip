// vqa_prior_attn.hip — the prior's factorized attention (gfx950): flash attention for the row and prev-row modes,
// the column mode, their backward passes, and the attention probabilities for inspection.
//
// Replaces (reference file:line):
//   src/transformer/factorized_attention.py:74-388      row / col / prev-row attention -> attn_*
//   src/transformer/transformer.py:106-115               attention_weights              -> attn_weights
#include "vqa_prior.h"

namespace vqa {

// ---------------------------------------------------------------------------------------------------
// Factorized attention (keras MultiHeadAttention core after the query/key/value EinsumDense; head dim 16).
// Q, K, V, O: (N, T, H*16) in the activation dtype; lse: (N, T, H) fp32 in the log2 domain (x = s*scale*log2e).
//   mode 0 row      (factorized_attention.py:74-141): causal inside each block of l positions
//   mode 1 col      (:210-286): position j of block b attends positions j of blocks 0..b (causal over blocks)
//   mode 2 prev-row (:308-388): block b attends every position of block b-1; block 0 sees the zero block,
//                   i.e. keys = key bias, values = value bias: O = value bias exactly
// Modes 0 and 2: flash attention on MFMA. A workgroup = 64 queries (wave w: 16); key tiles of 64 in LDS.
// S^T = K Q^T (K = head dim) leaves each lane 16 scores of ONE query (lane & 15), so softmax statistics are
// per-lane plus two cross-group shuffles; O^T = V^T P^T (K = keys) reads V^T by transposed LDS reads.
struct AttnArgs {
  const void* q;
  const void* k;
  const void* v;
  void* o;
  float* lse;
  const void* dout;
  float* dsum;  // D = rowsum(dO * O), written by attn_bwd_q, read by attn_bwd_kv
  void* dq;
  void* dk;
  void* dv;
  const float* vbias;  // mode 2: value bias (H*16), the block-0 output
  int N, T, H, l;
  float scale;
};

constexpr int AKS = AHD + 4;  // LDS row stride of a 64 x 16 tile (elements)

// 64 rows x 16 of (N, T, H*16) rows [r0, r0+64) of head h -> LDS tile [64][AKS]
template <class T>
__device__ __forceinline__ void stage64(T* dst, const T* src, long long row0, int H, int h) {
  const int r = threadIdx.x >> 2, q = (threadIdx.x & 3) * 4;
  const T* p = src + ((row0 + r) * H + h) * AHD + q;
  if constexpr (sizeof(T) == 2) *(uint2*)(dst + r * AKS + q) = *(const uint2*)p;
  else *(uint4*)(dst + r * AKS + q) = *(const uint4*)p;
}

// the calling thread's 4-element chunk of a 64 x 16 tile, held in registers between the global load (issued one
// tile ahead) and the LDS store
template <class T> struct Chunk64 {
  typedef typename std::conditional<sizeof(T) == 2, uint2, uint4>::type V;
  V v;
  __device__ __forceinline__ void load(const T* src, long long row0, int H, int h) {
    const int r = threadIdx.x >> 2, q = (threadIdx.x & 3) * 4;
    v = *(const V*)(src + ((row0 + r) * H + h) * AHD + q);
  }
  __device__ __forceinline__ void store(T* dst) const {
    const int r = threadIdx.x >> 2, q = (threadIdx.x & 3) * 4;
    *(V*)(dst + r * AKS + q) = v;
  }
};

// Ceiling (row attention at SMALL_PRIOR, B = 8, ctx 8192, 2 heads, blocks of 2048): 134 M causal scores, each
// one v_exp_f32 (8 issue cycles per 64 lanes) plus ~4 other VALU (scale FMA, max, sum, bf16 pack) -> about
// 20 us on 256 CUs; the QK / PV MFMAs (head dim 16, K = 16) are < 10 % of that. Measured 64 us (r2g/r3). A
// single-wave-per-64-queries form without workgroup barriers (4 query groups per staged key tile) measured
// 69.5 us: at 8 waves per CU the per-wave serial chain of the online softmax is not hidden, where this form
// keeps 32 waves per CU.
template <class T, int MODE>
__global__ __launch_bounds__(256) void attn_fwd_kernel(AttnArgs a) {
  typedef Att<T> A;
  __shared__ __attribute__((aligned(16))) T Ks[64 * AKS];
  __shared__ __attribute__((aligned(16))) T Vs[64 * AKS];
  const int qt = blockIdx.x, h = blockIdx.y, n = blockIdx.z, q0 = qt * 64, b = q0 / a.l;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), li = lane & 15, g = lane >> 4;
  const int qi = q0 + wave * 16 + li;
  const long long qrow = (long long)n * a.T + qi;
  T* orow = (T*)a.o + (qrow * a.H + h) * AHD + 4 * g;
  if (MODE == 2 && b == 0) {  // the zero block: uniform weights over identical (bias) values
    f32x4 v = *(const f32x4*)(a.vbias + h * AHD + 4 * g);
    st4(orow, v);
    if (g == 0) a.lse[qrow * a.H + h] = 0.f;
    return;
  }
  const typename A::dfrag qf = A::ld_d((const T*)a.q + (qrow * a.H + h) * AHD);
  const int kt0 = MODE == 0 ? b * a.l / 64 : (b - 1) * a.l / 64, kt1 = MODE == 0 ? qt : b * a.l / 64 - 1;
  const float c = a.scale * kLog2e;
  float m = -INFINITY, lsum = 0.f;
  f32x4 oacc = {0.f, 0.f, 0.f, 0.f};
  Chunk64<T> ck, cv;
  ck.load((const T*)a.k, (long long)n * a.T + kt0 * 64, a.H, h);
  cv.load((const T*)a.v, (long long)n * a.T + kt0 * 64, a.H, h);
  for (int kt = kt0; kt <= kt1; ++kt) {
    __syncthreads();
    ck.store(Ks);
    cv.store(Vs);
    __syncthreads();
    if (kt < kt1) {  // next tile in flight while this one computes
      ck.load((const T*)a.k, (long long)n * a.T + (kt + 1) * 64, a.H, h);
      cv.load((const T*)a.v, (long long)n * a.T + (kt + 1) * 64, a.H, h);
    }
    // raw scores; the scale (> 0) is applied inside the exponent: p = 2^(s*c - m), m = max(s)*c
    float x[4][4];
    float mt = -INFINITY;
    const bool diag = MODE == 0 && kt == qt;
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const f32x4 s = A::mm_d(A::ld_d(Ks + (st * 16 + li) * AKS), qf, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
      for (int i = 0; i < 4; ++i) x[st][i] = s[i];
    }
    if (diag) {
#pragma unroll
      for (int st = 0; st < 4; ++st)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (st * 16 + 4 * g + i > wave * 16 + li) x[st][i] = -INFINITY;
    }
#pragma unroll
    for (int st = 0; st < 4; ++st)
      mt = fmaxf(fmaxf(fmaxf(mt, x[st][0]), fmaxf(x[st][1], x[st][2])), x[st][3]);
    mt = grp_max(mt) * c;
    const float mn = fmaxf(m, mt), alpha = fexp2(m - mn);
    m = mn;
    float p[4][4], ps = 0.f;
#pragma unroll
    for (int st = 0; st < 4; ++st)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        p[st][i] = fexp2(__builtin_fmaf(x[st][i], c, -mn));
        ps += p[st][i];
      }
    lsum = lsum * alpha + ps;
    oacc = oacc * alpha;
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      const float p8[8] = {p[2 * cc][0], p[2 * cc][1], p[2 * cc][2], p[2 * cc][3],
                           p[2 * cc + 1][0], p[2 * cc + 1][1], p[2 * cc + 1][2], p[2 * cc + 1][3]};
      oacc = A::mm_rows(Vs, AKS, 32 * cc, p8, oacc);
    }
  }
  const float lt = grp_sum(lsum), inv = 1.0f / lt;
  st4(orow, oacc * inv);
  if (g == 0) a.lse[qrow * a.H + h] = m + log2f(lt);
}

template <class T, int MODE>
__global__ __launch_bounds__(256) void attn_bwd_q_kernel(AttnArgs a) {
  typedef Att<T> A;
  __shared__ __attribute__((aligned(16))) T Ks[64 * AKS];
  __shared__ __attribute__((aligned(16))) T Vs[64 * AKS];
  const int qt = blockIdx.x, h = blockIdx.y, n = blockIdx.z, q0 = qt * 64, b = q0 / a.l;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), li = lane & 15, g = lane >> 4;
  const int qi = q0 + wave * 16 + li;
  const long long qrow = (long long)n * a.T + qi, off = (qrow * a.H + h) * AHD;
  // D = rowsum(dO * O)
  const f32x4 dov = ld4((const T*)a.dout + off + 4 * g), ov = ld4((const T*)a.o + off + 4 * g);
  const float D = grp_sum(dov[0] * ov[0] + dov[1] * ov[1] + dov[2] * ov[2] + dov[3] * ov[3]);
  if (g == 0) a.dsum[qrow * a.H + h] = D;
  T* dqrow = (T*)a.dq + off + 4 * g;
  if (MODE == 2 && b == 0) {  // constant scores: no gradient reaches the queries
    st4(dqrow, f32x4{0.f, 0.f, 0.f, 0.f});
    return;
  }
  const typename A::dfrag qf = A::ld_d((const T*)a.q + off), dof = A::ld_d((const T*)a.dout + off);
  const float lse = a.lse[qrow * a.H + h];
  const int kt0 = MODE == 0 ? b * a.l / 64 : (b - 1) * a.l / 64, kt1 = MODE == 0 ? qt : b * a.l / 64 - 1;
  const float c = a.scale * kLog2e;
  f32x4 dqacc = {0.f, 0.f, 0.f, 0.f};
  Chunk64<T> ck, cv;
  ck.load((const T*)a.k, (long long)n * a.T + kt0 * 64, a.H, h);
  cv.load((const T*)a.v, (long long)n * a.T + kt0 * 64, a.H, h);
  for (int kt = kt0; kt <= kt1; ++kt) {
    __syncthreads();
    ck.store(Ks);
    cv.store(Vs);
    __syncthreads();
    if (kt < kt1) {
      ck.load((const T*)a.k, (long long)n * a.T + (kt + 1) * 64, a.H, h);
      cv.load((const T*)a.v, (long long)n * a.T + (kt + 1) * 64, a.H, h);
    }
    float ds[4][4];
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const f32x4 s = A::mm_d(A::ld_d(Ks + (st * 16 + li) * AKS), qf, f32x4{0.f, 0.f, 0.f, 0.f});
      const f32x4 dp = A::mm_d(A::ld_d(Vs + (st * 16 + li) * AKS), dof, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float p = fexp2(__builtin_fmaf(s[i], c, -lse));
        if (MODE == 0 && kt == qt && st * 16 + 4 * g + i > wave * 16 + li) p = 0.f;
        ds[st][i] = p * (dp[i] - D);
      }
    }
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      const float p8[8] = {ds[2 * cc][0], ds[2 * cc][1], ds[2 * cc][2], ds[2 * cc][3],
                           ds[2 * cc + 1][0], ds[2 * cc + 1][1], ds[2 * cc + 1][2], ds[2 * cc + 1][3]};
      dqacc = A::mm_rows(Ks, AKS, 32 * cc, p8, dqacc);
    }
  }
  st4(dqrow, dqacc * a.scale);
}

template <class T, int MODE>
__global__ __launch_bounds__(256) void attn_bwd_kv_kernel(AttnArgs a) {
  typedef Att<T> A;
  __shared__ __attribute__((aligned(16))) T Qs[64 * AKS];
  __shared__ __attribute__((aligned(16))) T Ds[64 * AKS];  // dO tile
  __shared__ __attribute__((aligned(16))) float Ls[64];
  __shared__ __attribute__((aligned(16))) float Dd[64];
  const int kt = blockIdx.x, h = blockIdx.y, n = blockIdx.z, k0 = kt * 64, b = k0 / a.l;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), li = lane & 15, g = lane >> 4;
  const int ki = k0 + wave * 16 + li;
  const long long krow = (long long)n * a.T + ki, off = (krow * a.H + h) * AHD;
  T* dkrow = (T*)a.dk + off + 4 * g;
  T* dvrow = (T*)a.dv + off + 4 * g;
  const int nblk = a.T / a.l;
  int qt0, qt1;
  if (MODE == 0) {
    qt0 = kt;
    qt1 = (b + 1) * a.l / 64 - 1;
  } else {
    qt0 = (b + 1) * a.l / 64;
    qt1 = b + 1 < nblk ? (b + 2) * a.l / 64 - 1 : qt0 - 1;
  }
  const typename A::dfrag kf = A::ld_d((const T*)a.k + off), vf = A::ld_d((const T*)a.v + off);
  const float c = a.scale * kLog2e;
  f32x4 dkacc = {0.f, 0.f, 0.f, 0.f}, dvacc = {0.f, 0.f, 0.f, 0.f};
  Chunk64<T> cq, cd;
  float pl = 0.f, pd = 0.f;
  auto load_q = [&](int qt) {
    const long long r0 = (long long)n * a.T + qt * 64;
    cq.load((const T*)a.q, r0, a.H, h);
    cd.load((const T*)a.dout, r0, a.H, h);
    if (threadIdx.x < 64) {
      pl = a.lse[(r0 + threadIdx.x) * a.H + h];
      pd = a.dsum[(r0 + threadIdx.x) * a.H + h];
    }
  };
  if (qt0 <= qt1) load_q(qt0);
  for (int qt = qt0; qt <= qt1; ++qt) {
    __syncthreads();
    cq.store(Qs);
    cd.store(Ds);
    if (threadIdx.x < 64) {
      Ls[threadIdx.x] = pl;
      Dd[threadIdx.x] = pd;
    }
    __syncthreads();
    if (qt < qt1) load_q(qt + 1);
    float p[4][4], ds[4][4];
#pragma unroll
    for (int qs = 0; qs < 4; ++qs) {
      const f32x4 s = A::mm_d(A::ld_d(Qs + (qs * 16 + li) * AKS), kf, f32x4{0.f, 0.f, 0.f, 0.f});
      const f32x4 dp = A::mm_d(A::ld_d(Ds + (qs * 16 + li) * AKS), vf, f32x4{0.f, 0.f, 0.f, 0.f});
      // the 4 query rows' lse and D: one 16-byte LDS read each
      const f32x4 lq = *(const f32x4*)(Ls + qs * 16 + 4 * g), dq = *(const f32x4*)(Dd + qs * 16 + 4 * g);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ql = qs * 16 + 4 * g + i;
        float pv = fexp2(__builtin_fmaf(s[i], c, -lq[i]));
        if (MODE == 0 && qt == kt && wave * 16 + li > ql) pv = 0.f;
        p[qs][i] = pv;
        ds[qs][i] = pv * (dp[i] - dq[i]);
      }
    }
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      const float p8[8] = {p[2 * cc][0], p[2 * cc][1], p[2 * cc][2], p[2 * cc][3],
                           p[2 * cc + 1][0], p[2 * cc + 1][1], p[2 * cc + 1][2], p[2 * cc + 1][3]};
      const float d8[8] = {ds[2 * cc][0], ds[2 * cc][1], ds[2 * cc][2], ds[2 * cc][3],
                           ds[2 * cc + 1][0], ds[2 * cc + 1][1], ds[2 * cc + 1][2], ds[2 * cc + 1][3]};
      dvacc = A::mm_rows(Ds, AKS, 32 * cc, p8, dvacc);
      dkacc = A::mm_rows(Qs, AKS, 32 * cc, d8, dkacc);
    }
  }
  st4(dkrow, dkacc * a.scale);
  st4(dvrow, dvacc);
}

// mode 1 (column attention, blocks <= 8): one thread per (item, position in block, head); all NB rows of the
// column in registers. Forward writes O and lse; backward writes dQ, dK, dV of the whole column (no atomics).
template <class T, int NB>
__global__ __launch_bounds__(256) void attn_col_fwd_kernel(AttnArgs a) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)a.N * a.l * a.H) return;
  const int h = (int)(e % a.H), j = (int)((e / a.H) % a.l);
  const long long n = e / ((long long)a.H * a.l);
  auto off = [&](int b) { return (((long long)n * a.T + (long long)b * a.l + j) * a.H + h) * AHD; };
  float kk[NB][AHD];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int d = 0; d < AHD; d += 4) {
      const f32x4 v = ld4((const T*)a.k + off(b) + d);
      kk[b][d] = v[0]; kk[b][d + 1] = v[1]; kk[b][d + 2] = v[2]; kk[b][d + 3] = v[3];
    }
  const float c = a.scale * kLog2e;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    float q[AHD];
#pragma unroll
    for (int d = 0; d < AHD; d += 4) {
      const f32x4 v = ld4((const T*)a.q + off(b) + d);
      q[d] = v[0]; q[d + 1] = v[1]; q[d + 2] = v[2]; q[d + 3] = v[3];
    }
    float x[NB], m = -INFINITY;
#pragma unroll
    for (int bb = 0; bb <= b; ++bb) {
      float s = 0.f;
#pragma unroll
      for (int d = 0; d < AHD; ++d) s += q[d] * kk[bb][d];
      x[bb] = s * c;
      m = fmaxf(m, x[bb]);
    }
    float l = 0.f, o[AHD];
#pragma unroll
    for (int d = 0; d < AHD; ++d) o[d] = 0.f;
#pragma unroll
    for (int bb = 0; bb <= b; ++bb) {
      const float p = exp2f(x[bb] - m);
      l += p;
#pragma unroll
      for (int d = 0; d < AHD; d += 4) {
        const f32x4 v = ld4((const T*)a.v + off(bb) + d);
        o[d] += p * v[0]; o[d + 1] += p * v[1]; o[d + 2] += p * v[2]; o[d + 3] += p * v[3];
      }
    }
    const float inv = 1.0f / l;
#pragma unroll
    for (int d = 0; d < AHD; d += 4)
      st4((T*)a.o + off(b) + d, f32x4{o[d] * inv, o[d + 1] * inv, o[d + 2] * inv, o[d + 3] * inv});
    a.lse[(off(b) / AHD)] = m + log2f(l);
  }
}

template <class T, int NB>
__global__ __launch_bounds__(256) void attn_col_bwd_kernel(AttnArgs a) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)a.N * a.l * a.H) return;
  const int h = (int)(e % a.H), j = (int)((e / a.H) % a.l);
  const long long n = e / ((long long)a.H * a.l);
  auto off = [&](int b) { return (((long long)n * a.T + (long long)b * a.l + j) * a.H + h) * AHD; };
  auto ldrow = [&](const void* base, int b, float (&r)[AHD]) {
#pragma unroll
    for (int d = 0; d < AHD; d += 4) {
      const f32x4 v = ld4((const T*)base + off(b) + d);
      r[d] = v[0]; r[d + 1] = v[1]; r[d + 2] = v[2]; r[d + 3] = v[3];
    }
  };
  const float c = a.scale * kLog2e;
  // P and dS for the column (lower triangle)
  float P[NB][NB], dS[NB][NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    float q[AHD], go[AHD];
    ldrow(a.q, b, q);
    ldrow(a.dout, b, go);
    const float lse = a.lse[off(b) / AHD];
    float D = 0.f;
#pragma unroll
    for (int bb = 0; bb <= b; ++bb) {
      float kr[AHD], vr[AHD];
      ldrow(a.k, bb, kr);
      ldrow(a.v, bb, vr);
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int d = 0; d < AHD; ++d) {
        s += q[d] * kr[d];
        dp += go[d] * vr[d];
      }
      P[b][bb] = exp2f(s * c - lse);
      dS[b][bb] = dp;
      D += P[b][bb] * dp;
    }
#pragma unroll
    for (int bb = 0; bb <= b; ++bb) dS[b][bb] = P[b][bb] * (dS[b][bb] - D);
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    // dQ_b = scale * sum_{bb <= b} dS[b][bb] k_bb ; dK_b = scale * sum_{bq >= b} dS[bq][b] q_bq ;
    // dV_b = sum_{bq >= b} P[bq][b] dO_bq
    float dq[AHD], dk[AHD], dv[AHD];
#pragma unroll
    for (int d = 0; d < AHD; ++d) dq[d] = dk[d] = dv[d] = 0.f;
#pragma unroll
    for (int bb = 0; bb <= b; ++bb) {
      float kr[AHD];
      ldrow(a.k, bb, kr);
#pragma unroll
      for (int d = 0; d < AHD; ++d) dq[d] += dS[b][bb] * kr[d];
    }
#pragma unroll
    for (int bq = b; bq < NB; ++bq) {
      float q[AHD], go[AHD];
      ldrow(a.q, bq, q);
      ldrow(a.dout, bq, go);
#pragma unroll
      for (int d = 0; d < AHD; ++d) {
        dk[d] += dS[bq][b] * q[d];
        dv[d] += P[bq][b] * go[d];
      }
    }
#pragma unroll
    for (int d = 0; d < AHD; d += 4) {
      st4((T*)a.dq + off(b) + d, f32x4{dq[d], dq[d + 1], dq[d + 2], dq[d + 3]} * a.scale);
      st4((T*)a.dk + off(b) + d, f32x4{dk[d], dk[d + 1], dk[d + 2], dk[d + 3]} * a.scale);
      st4((T*)a.dv + off(b) + d, f32x4{dv[d], dv[d + 1], dv[d + 2], dv[d + 3]});
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// Attention probabilities for inspection (transformer.py:106-115 attention_weights; the layouts keras
// MultiHeadAttention(return_attention_scores=True) gives factorized_attention.py:121-135, 260-284, 355-386 at a
// whole number of blocks): p = 2^(s*c - lse) recomputed from q, k and the lse the forward saved, fp32 out.
// Store-bound (N*H*T*l floats for modes 0 / 2); every element of w is written exactly once, masked ones as +0.
struct AttnWArgs {
  const void* q;
  const void* k;
  const float* lse;
  float* w;
  int N, T, H, l;
  float scale;
  float uniform;  // 1.0f / l: every weight of mode 2's block 0 (identical bias keys)
};

constexpr int AWS = 64 + 4;  // LDS row stride (floats) of a wave's 16 x 64 probability tile

// Modes 0 and 2, w (N*nb, H, l, l). The forward's tiling: a workgroup = 64 queries (wave w: 16), key tiles of 64
// staged in LDS, S^T = K Q^T on the same MFMA, so a lane holds 4 consecutive keys of ONE query — a wave store of
// the accumulator as it stands would be 16 rows x 64 B. The wave's 16 x 64 tile goes through its own LDS tile
// instead and leaves as 4 instructions of 4 rows x 256 B (16 lanes x 16 B along each row); over the key loop a
// wave writes its 16 output rows whole. Tiles past the diagonal (mode 0) and block 0 (mode 2) are constant fills
// with the same map: no q, k or lse is read for them.
template <class T, int MODE>
__global__ __launch_bounds__(256) void attn_weights_kernel(AttnWArgs a) {
  typedef Att<T> A;
  __shared__ __attribute__((aligned(16))) T Ks[64 * AKS];
  __shared__ __attribute__((aligned(16))) float Ps[4][16 * AWS];
  const int qt = blockIdx.x, h = blockIdx.y, n = blockIdx.z, q0 = qt * 64, b = q0 / a.l;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), li = lane & 15, g = lane >> 4;
  const int nt = a.l / 64;  // key tiles per output row
  // the wave's 16 output rows: batch item n*nb + b, head h, rows q0 - b*l + 16*wave ..; 64-bit from here on
  const long long blk = ((long long)n * (a.T / a.l) + b) * a.H + h;
  float* wrow = a.w + (blk * a.l + (q0 - b * a.l + wave * 16)) * (long long)a.l;
  const int sr = lane >> 4, sc = 4 * (lane & 15);  // store map: pass r writes row 4r + sr, columns sc .. sc+3
  auto fill = [&](int t, float v) {
#pragma unroll
    for (int r = 0; r < 4; ++r) *(f32x4*)(wrow + (long long)(4 * r + sr) * a.l + t * 64 + sc) = f32x4{v, v, v, v};
  };
  if (MODE == 2 && b == 0) {  // the zero block: uniform weights; its lse is a placeholder and is not read
    for (int t = 0; t < nt; ++t) fill(t, a.uniform);
    return;
  }
  const long long qrow = (long long)n * a.T + q0 + wave * 16 + li;
  const typename A::dfrag qf = A::ld_d((const T*)a.q + (qrow * a.H + h) * AHD);
  const float lse = a.lse[qrow * a.H + h];
  const int kt0 = MODE == 0 ? b * nt : (b - 1) * nt, tl = MODE == 0 ? qt - kt0 : nt - 1;  // last tile with scores
  const float c = a.scale * kLog2e;
  float* P = Ps[wave];
  Chunk64<T> ck;
  ck.load((const T*)a.k, (long long)n * a.T + kt0 * 64, a.H, h);
  for (int t = 0; t <= tl; ++t) {
    __syncthreads();
    ck.store(Ks);
    __syncthreads();
    if (t < tl) ck.load((const T*)a.k, (long long)n * a.T + (kt0 + t + 1) * 64, a.H, h);
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const f32x4 s = A::mm_d(A::ld_d(Ks + (st * 16 + li) * AKS), qf, f32x4{0.f, 0.f, 0.f, 0.f});
      f32x4 p;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        p[i] = fexp2(__builtin_fmaf(s[i], c, -lse));
        if (MODE == 0 && t == tl && st * 16 + 4 * g + i > wave * 16 + li) p[i] = 0.f;
      }
      *(f32x4*)(P + li * AWS + st * 16 + 4 * g) = p;
    }
    // the tile is the wave's own: a wave's LDS traffic is processed in order, the fences keep the compiler's order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int r = 0; r < 4; ++r)
      *(f32x4*)(wrow + (long long)(4 * r + sr) * a.l + t * 64 + sc) = *(const f32x4*)(P + (4 * r + sr) * AWS + sc);
    // the next tile's writes to P come after the loop's barriers
  }
  for (int t = tl + 1; t < nt; ++t) fill(t, 0.f);
}

// Mode 1, w (N*l, H, nb, nb): thread e = (n*l + j)*H + h of attn_col_fwd_kernel owns the nb x nb matrix at
// w + e*nb*nb, so a workgroup's 256 matrices are one contiguous run that starts on a 16-byte boundary whatever nb
// is. Rows of nb <= 8 floats cannot be 16-byte stores per thread (nb*nb is odd for odd nb): the matrices are
// transposed through LDS and the workgroup streams the run out, lane f writing floats 4f .. 4f+3 (a wave: 1 KiB
// contiguous); only the last workgroup can end in a tail of fewer than 4 floats. Scores as the column forward forms
// them (the same sequential dot product), p = exp2(s*c - lse) as attn_col_bwd_kernel.
template <class T, int NB>
__global__ __launch_bounds__(256) void attn_col_weights_kernel(AttnWArgs a) {
  constexpr int M = NB * NB;
  __shared__ __attribute__((aligned(16))) float Ws[M * 256];  // [m][(t + m) & 255]: conflict-free both ways
  const long long total = (long long)a.N * a.l * a.H, e0 = (long long)blockIdx.x * 256, e = e0 + threadIdx.x;
  if (e < total) {
    const int h = (int)(e % a.H), j = (int)((e / a.H) % a.l);
    const long long n = e / ((long long)a.H * a.l);
    auto off = [&](int b) { return (((long long)n * a.T + (long long)b * a.l + j) * a.H + h) * AHD; };
    float kk[NB][AHD];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int d = 0; d < AHD; d += 4) {
        const f32x4 v = ld4((const T*)a.k + off(b) + d);
        kk[b][d] = v[0]; kk[b][d + 1] = v[1]; kk[b][d + 2] = v[2]; kk[b][d + 3] = v[3];
      }
    const float c = a.scale * kLog2e;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      float q[AHD];
#pragma unroll
      for (int d = 0; d < AHD; d += 4) {
        const f32x4 v = ld4((const T*)a.q + off(b) + d);
        q[d] = v[0]; q[d + 1] = v[1]; q[d + 2] = v[2]; q[d + 3] = v[3];
      }
      const float lse = a.lse[off(b) / AHD];
#pragma unroll
      for (int bb = 0; bb < NB; ++bb) {
        float p = 0.f;
        if (bb <= b) {
          float s = 0.f;
#pragma unroll
          for (int d = 0; d < AHD; ++d) s += q[d] * kk[bb][d];
          p = exp2f(s * c - lse);
        }
        const int m = b * NB + bb;
        Ws[m * 256 + ((threadIdx.x + m) & 255)] = p;
      }
    }
  }
  __syncthreads();
  const long long rest = total - e0;
  const int cnt = (int)(rest < 256 ? rest : 256) * M;  // floats of this workgroup's run
  float* out = a.w + e0 * M;
  auto at = [&](int f) { const int t = f / M, m = f - t * M; return Ws[m * 256 + ((t + m) & 255)]; };
  for (int f = threadIdx.x * 4; f < cnt; f += 1024) {
    if (f + 4 <= cnt) *(f32x4*)(out + f) = f32x4{at(f), at(f + 1), at(f + 2), at(f + 3)};
    else
      for (int u = f; u < cnt; ++u) out[u] = at(u);
  }
}

// ---------------------------------------------------------------------------------------------------
template <class T>
static int launch_attn(bool fwd, int mode, const AttnArgs& a, hipStream_t s) {
  const int nb = a.T / a.l;
  if (mode == 1) {
    const unsigned g = pr_grid((long long)a.N * a.l * a.H, 256, 1 << 30);
#define VQA_COL(NB)                                                                                         \
  case NB:                                                                                                  \
    if (fwd) hipLaunchKernelGGL((attn_col_fwd_kernel<T, NB>), dim3(g), dim3(256), 0, s, a);                 \
    else hipLaunchKernelGGL((attn_col_bwd_kernel<T, NB>), dim3(g), dim3(256), 0, s, a);                     \
    break;
    switch (nb) {
      VQA_COL(1) VQA_COL(2) VQA_COL(3) VQA_COL(4) VQA_COL(5) VQA_COL(6) VQA_COL(7) VQA_COL(8)
      default: set_error("attn: column attention supports 1..8 blocks (got %d)", nb); return VQA_E_UNSUPPORTED;
    }
#undef VQA_COL
    VQA_LAUNCHED("attn_col_kernel");
    return VQA_OK;
  }
  const dim3 grid(a.T / 64, a.H, a.N);
  if (fwd) {
    if (mode == 0) hipLaunchKernelGGL((attn_fwd_kernel<T, 0>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((attn_fwd_kernel<T, 2>), grid, dim3(256), 0, s, a);
    VQA_LAUNCHED("attn_fwd_kernel");
  } else {
    if (mode == 0) {
      hipLaunchKernelGGL((attn_bwd_q_kernel<T, 0>), grid, dim3(256), 0, s, a);
      hipLaunchKernelGGL((attn_bwd_kv_kernel<T, 0>), grid, dim3(256), 0, s, a);
    } else {
      hipLaunchKernelGGL((attn_bwd_q_kernel<T, 2>), grid, dim3(256), 0, s, a);
      hipLaunchKernelGGL((attn_bwd_kv_kernel<T, 2>), grid, dim3(256), 0, s, a);
    }
    VQA_LAUNCHED("attn_bwd_kernel");
  }
  return VQA_OK;
}

static int attn_check(int N, int T, int H, int head_dim, int l, int mode) {
  VQA_ARG(N > 0 && T > 0 && H > 0 && l > 0 && T % l == 0 && mode >= 0 && mode <= 2, "attn: bad shape");
  VQA_REQUIRE(head_dim == AHD, VQA_E_UNSUPPORTED, "attn: head_dim %d unsupported (16)", head_dim);
  VQA_REQUIRE(mode == 1 || l % 64 == 0, VQA_E_UNSUPPORTED, "attn: block length %d not a multiple of 64", l);
  return VQA_OK;
}

template <class T>
static int launch_attn_weights(int mode, const AttnWArgs& a, hipStream_t s) {
  if (mode == 1) {
    const unsigned g = (unsigned)(((long long)a.N * a.l * a.H + 255) / 256);
#define VQA_COLW(NB) \
  case NB: hipLaunchKernelGGL((attn_col_weights_kernel<T, NB>), dim3(g), dim3(256), 0, s, a); break;
    switch (a.T / a.l) { VQA_COLW(1) VQA_COLW(2) VQA_COLW(3) VQA_COLW(4) VQA_COLW(5) VQA_COLW(6) VQA_COLW(7) VQA_COLW(8) }
#undef VQA_COLW
    VQA_LAUNCHED("attn_col_weights_kernel");
    return VQA_OK;
  }
  const dim3 grid(a.T / 64, a.H, a.N);
  if (mode == 0) hipLaunchKernelGGL((attn_weights_kernel<T, 0>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((attn_weights_kernel<T, 2>), grid, dim3(256), 0, s, a);
  VQA_LAUNCHED("attn_weights_kernel");
  return VQA_OK;
}

}  // namespace vqa

using namespace vqa;

extern "C" int vqa_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse, const float* vbias, int N,
                            int T, int H, int head_dim, int l, int mode, float scale, int dtype, vqa_stream_t stream) {
  VQA_ARG(q && k && v && o && lse && pr_dt(dtype) && (mode != 2 || vbias), "attn_fwd: bad arguments");
  if (int rc = attn_check(N, T, H, head_dim, l, mode)) return rc;
  AttnArgs a{q, k, v, o, lse, nullptr, nullptr, nullptr, nullptr, nullptr, vbias, N, T, H, l, scale};
  hipStream_t s = (hipStream_t)stream;
  return dtype == VQA_BF16 ? launch_attn<bf16>(true, mode, a, s) : launch_attn<float>(true, mode, a, s);
}

extern "C" int vqa_attn_bwd(const void* q, const void* k, const void* v, const void* o, const float* lse,
                            const void* dout, float* dsum, void* dq, void* dk, void* dv, int N, int T, int H,
                            int head_dim, int l, int mode, float scale, int dtype, vqa_stream_t stream) {
  VQA_ARG(q && k && v && o && lse && dout && dq && dk && dv && pr_dt(dtype) && (mode == 1 || dsum),
          "attn_bwd: bad arguments");
  if (int rc = attn_check(N, T, H, head_dim, l, mode)) return rc;
  AttnArgs a{q, k, v, (void*)o, (float*)lse, dout, dsum, dq, dk, dv, nullptr, N, T, H, l, scale};
  hipStream_t s = (hipStream_t)stream;
  return dtype == VQA_BF16 ? launch_attn<bf16>(false, mode, a, s) : launch_attn<float>(false, mode, a, s);
}

extern "C" size_t vqa_attn_weights_elems(int N, int T, int H, int l, int mode) {
  if (!(N > 0 && T > 0 && H > 0 && l > 0 && T % l == 0 && mode >= 0 && mode <= 2)) return 0;
  const size_t nb = (size_t)(T / l), side = mode == 1 ? nb : (size_t)l, items = mode == 1 ? (size_t)l : nb;
  size_t e = 0;  // N * items * H * side * side
  if (__builtin_mul_overflow((size_t)N, items, &e) || __builtin_mul_overflow(e, (size_t)H, &e) ||
      __builtin_mul_overflow(e, side, &e) || __builtin_mul_overflow(e, side, &e))
    return 0;
  return e;
}

extern "C" int vqa_attn_weights(const void* q, const void* k, const float* lse, float* w, size_t w_elems, int N, int T,
                                int H, int head_dim, int l, int mode, float scale, int dtype, vqa_stream_t stream) {
  VQA_ARG(q && k && lse && w, "attn_weights: null q, k, lse or w");
  VQA_ARG(pr_dt(dtype), "attn_weights: dtype %d is neither VQA_F32 nor VQA_BF16", dtype);
  VQA_ARG(N > 0 && T > 0 && H > 0 && l > 0 && T % l == 0 && mode >= 0 && mode <= 2,
          "attn_weights: bad shape (N %d, T %d, H %d, l %d, mode %d)", N, T, H, l, mode);
  VQA_REQUIRE(head_dim == AHD, VQA_E_UNSUPPORTED, "attn_weights: head_dim %d unsupported (16)", head_dim);
  VQA_REQUIRE(mode == 1 || l % 64 == 0, VQA_E_UNSUPPORTED, "attn_weights: block length %d not a multiple of 64", l);
  VQA_REQUIRE(mode != 1 || T / l <= 8, VQA_E_UNSUPPORTED,
              "attn_weights: column attention supports 1..8 blocks (got %d)", T / l);
  VQA_ARG(std::isfinite(scale) && scale > 0.f, "attn_weights: scale %g is not finite and positive", (double)scale);
  const size_t want = vqa_attn_weights_elems(N, T, H, l, mode);
  VQA_ARG(want != 0 && w_elems == want, "attn_weights: w holds %zu elements, the layout of mode %d has %zu", w_elems,
          mode, want);
  VQA_ARG((reinterpret_cast<uintptr_t>(w) & 15) == 0, "attn_weights: w is not 16-byte aligned");
  VQA_ARG(mode == 1 ? ((long long)N * l * H + 255) / 256 <= 0x7fffffffLL : (N <= 65535 && H <= 65535),
          "attn_weights: N %d or H %d beyond the launch grid", N, H);
  AttnWArgs a{q, k, lse, w, N, T, H, l, scale, 1.0f / (float)l};
  hipStream_t s = (hipStream_t)stream;
  return dtype == VQA_BF16 ? launch_attn_weights<bf16>(mode, a, s) : launch_attn_weights<float>(mode, a, s);
}
