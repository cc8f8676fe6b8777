// vqa_prior_seqlin.hip — the prior's sequence-linear layers (gfx950): forward, data gradient, weight preparation
// and weight gradient.
//
// Replaces (reference file:line):
//   src/transformer/factorized_attention.py:36          Conv1D(3w, 3, padding="causal") -> seqlin (3 taps)
//   keras MultiHeadAttention query/key/value/output EinsumDense, proj / mlp Dense      -> seqlin (1 tap)
#include "vqa_prior.h"

namespace vqa {

// ---------------------------------------------------------------------------------------------------
// Sequence-linear layer (MFMA): Y[r][n] = sum_tap sum_k X[src(r, tap)][k] * Wv[tap][k][n] + b[n] (+ R[r][n])
//   src(r, tap) = the row of the same sequence at time t + dir * (taps - 1 - tap); rows outside [0, T) are zero.
//   dir = -1, taps = 3: Conv1D(k=3, padding="causal") forward; dir = +1 with the transposed weight view: its
//   data gradient. taps = 1: Dense / EinsumDense (and their data gradients with wtrans = 1).
//   Wv[tap][k][n] = wtrans ? w[(tap*N + n)*K + k] : w[(tap*K + k)*N + n]
// Workgroup = 128 rows of one sequence; wave w owns rows 32w .. 32w+31 (two 16-row MFMA column tiles) and
// every 16-wide output tile. Operands: A = Wv^T (staged in LDS per tap, output channel rows), B = X^T (row
// tile in LDS); the output D[n][row] gives each lane 4 consecutive channels of one row.
struct SeqLinArgs {
  const void* x;
  const float* w;
  const void* wp;  // optional: weights prepared by vqa_seqlin_prep as [taps][N][K] in the activation dtype
  const float* b;
  const void* r;
  void* y;
  long long ldx, ldr, ldy;
  int nseq, T, K, N, taps, dir, wtrans, accumulate, tiles_per_seq;
  const float* lng;  // optional (seqlin_d, bf16, K = 128): LayerNorm(gamma, beta, eps) of each input row first
  const float* lnb;
  float lneps;
};

constexpr int kSlRows = 128;

template <class T, int NT>
__global__ __launch_bounds__(256) void seqlin_kernel(SeqLinArgs a) {
  typedef Mfma<T> M;
  constexpr int PAD = 16 / (int)sizeof(T);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int KS = a.K + PAD;  // LDS row stride (elements) of both tiles
  T* Wt = (T*)smem;          // [N][K + PAD]
  const int halo = a.taps - 1, lo = a.dir < 0 ? halo : 0;
  T* X = Wt + a.N * KS;      // [kSlRows + halo][K + PAD]; row j <-> time t0 - lo + j
  const int seq = blockIdx.x / a.tiles_per_seq, t0 = (blockIdx.x - seq * a.tiles_per_seq) * kSlRows;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // stage the row tile (16-byte chunks; zeros outside the sequence)
  {
    constexpr int VEC = 16 / (int)sizeof(T);
    const int cpr = a.K / VEC, rows = kSlRows + halo;
    for (int e = threadIdx.x; e < rows * cpr; e += 256) {
      const int j = e / cpr, q = e - j * cpr, t = t0 - lo + j;
      uint4 v = {0u, 0u, 0u, 0u};
      if (t >= 0 && t < a.T) v = *(const uint4*)((const T*)a.x + ((long long)seq * a.T + t) * a.ldx + q * VEC);
      *(uint4*)(X + j * KS + q * VEC) = v;
    }
  }
  f32x4 acc[2][NT];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[s][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int kof = M::koff(lane), col = lane & 15;
  for (int tap = 0; tap < a.taps; ++tap) {
    if (tap) __syncthreads();  // every read of the previous tap's weights is done
    if (a.wp) {  // prepared image rows: straight 16-byte copies
      constexpr int VEC = 16 / (int)sizeof(T);
      const T* wp = (const T*)a.wp + (size_t)tap * a.K * a.N;
      const int cpr = a.K / VEC;
      for (int e = threadIdx.x; e < a.N * cpr; e += 256) {
        const int n = e / cpr, q = e - n * cpr;
        *(uint4*)(Wt + n * KS + q * VEC) = *(const uint4*)(wp + (size_t)n * a.K + q * VEC);
      }
    } else {
    const float* w = a.w + (size_t)tap * a.K * a.N;
    // 16-byte coalesced weight reads (4 consecutive elements of the contiguous axis)
    for (int e4 = threadIdx.x; e4 < a.K * a.N / 4; e4 += 256) {
      const f32x4 v = *(const f32x4*)(w + 4 * e4);
      if (a.wtrans) {  // w[n][k]: 4 consecutive k of one n
        const int n = 4 * e4 / a.K, k = 4 * e4 - n * a.K;
        st4(Wt + n * KS + k, v);
      } else {         // w[k][n]: 4 consecutive n of one k
        const int k = 4 * e4 / a.N, n = 4 * e4 - k * a.N;
#pragma unroll
        for (int i = 0; i < 4; ++i) Wt[(n + i) * KS + k] = (T)v[i];
      }
    }
    }
    __syncthreads();
    // row j of X for output row i: i + dir * (taps - 1 - tap) + lo
    const int sh = a.dir * (a.taps - 1 - tap) + lo;
    const T* xb0 = X + (wave * 32 + col + sh) * KS + kof;
    const T* wb = Wt + col * KS + kof;
    for (int kc = 0; kc < a.K; kc += M::KS) {
      const typename M::frag b0 = M::load(xb0 + kc), b1 = M::load(xb0 + 16 * KS + kc);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        if (nt * 16 >= a.N) break;
        const typename M::frag af = M::load(wb + nt * 16 * KS + kc);
        acc[0][nt] = M::mma(af, b0, acc[0][nt]);
        acc[1][nt] = M::mma(af, b1, acc[1][nt]);
      }
    }
  }
  // epilogue: lane (row = col, g) holds channels nt*16 + 4g .. +3
  const int g4 = 4 * (lane >> 4);
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int t = t0 + wave * 32 + s * 16 + col;
    if (t >= a.T) continue;
    const long long row = (long long)seq * a.T + t;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      if (nt * 16 >= a.N) break;
      const int c = nt * 16 + g4;
      f32x4 v = acc[s][nt];
      if (a.b) v = v + f32x4{a.b[c], a.b[c + 1], a.b[c + 2], a.b[c + 3]};
      if (a.r) v = v + ld4((const T*)a.r + row * a.ldr + c);
      T* yp = (T*)a.y + row * a.ldy + c;
      if (a.accumulate) v = v + ld4((const T*)yp);
      st4(yp, v);
    }
  }
}

// 4 consecutive activation elements kept raw (bf16: 8 bytes, fp32: 16 bytes) and widened when used
template <class T> struct RawR4;
template <> struct RawR4<bf16> {
  typedef uint2 type;
  type v;
  __device__ __forceinline__ f32x4 f() const {
    const bf16x4 b = __builtin_bit_cast(bf16x4, v);
    return f32x4{(float)b[0], (float)b[1], (float)b[2], (float)b[3]};
  }
};
template <> struct RawR4<float> {
  typedef uint4 type;
  type v;
  __device__ __forceinline__ f32x4 f() const { return __builtin_bit_cast(f32x4, v); }
};

// Persistent direct form for prepared weights (the prior's shapes, K and taps compile-time): the weight images
// of every tap staged ONCE per workgroup in LDS; each wave takes 16 rows of a 64-row tile and loads its B
// fragments (X^T: lane (row, g) <- 8 consecutive channels of its row) straight from global memory into
// registers — no LDS copy of X, no barrier per tile — with the NEXT tile's fragments and residual rows
// loaded while the current tile's MFMAs and stores run. The 1-tap epilogue goes through a per-wave fp32 LDS tile
// (16 rows x N) so that bias, residual and the store run on row-contiguous 16-byte chunks (whole rows per
// store instruction) instead of 4-channel pieces of 16 rows.
constexpr int kSdEpad = 4;

// 16 bytes of activations <-> VEC / 4 groups of 4 fp32
template <class T> __device__ __forceinline__ void chunk_widen(const uint4& u, f32x4* v) {
  if constexpr (sizeof(T) == 2) {
    const bf16x8 b = __builtin_bit_cast(bf16x8, u);
    v[0] = f32x4{(float)b[0], (float)b[1], (float)b[2], (float)b[3]};
    v[1] = f32x4{(float)b[4], (float)b[5], (float)b[6], (float)b[7]};
  } else {
    v[0] = __builtin_bit_cast(f32x4, u);
  }
}
template <class T> __device__ __forceinline__ uint4 chunk_narrow(const f32x4* v) {
  if constexpr (sizeof(T) == 2) {
    const bf16x8 b = {(bf16)v[0][0], (bf16)v[0][1], (bf16)v[0][2], (bf16)v[0][3],
                      (bf16)v[1][0], (bf16)v[1][1], (bf16)v[1][2], (bf16)v[1][3]};
    return __builtin_bit_cast(uint4, b);
  } else {
    return __builtin_bit_cast(uint4, v[0]);
  }
}

// LayerNorm of one row held as the B fragments of a 128-channel row (bf16, lane (row, g) holds channels
// 32 kc + 8 g .. +7 in fragment kc): the same arithmetic as layernorm8_fwd_kernel<bf16, 16> (vqa_cond.hip) —
// per-chunk sequential sums, then its pairwise sums over the 16 chunks, chunk bit 0 first (xl::grp_sum<16>; chunk
// bits 1, 0 are lane bits 5, 4 here, chunk bits 3, 2 the fragment index bits 1, 0) — so the fused and the unfused
// forms are bit-identical.
__device__ __forceinline__ void ln_row_frags(bf16x8 (&x)[4], const float* gs, const float* bs, int g8, float eps) {
  // the bf16 inputs are re-widened per pass (cheap) rather than held as 32 fp32 registers
  auto bfly = [](const float (&c)[4]) {
    float t[4];
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) t[kc] = xl::sum32(xl::sum16(c[kc]));  // chunk bits 0, 1
    return (t[0] + t[1]) + (t[2] + t[3]);                                 // chunk bits 2, 3
  };
  float s[4];
#pragma unroll
  for (int kc = 0; kc < 4; ++kc) {
    s[kc] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s[kc] += (float)x[kc][i];
  }
  const float mean = bfly(s) / 128.f;
#pragma unroll
  for (int kc = 0; kc < 4; ++kc) {
    s[kc] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float d = (float)x[kc][i] - mean;
      s[kc] += d * d;
    }
  }
  const float inv = 1.0f / sqrtf(bfly(s) / 128.f + eps);
#pragma unroll
  for (int kc = 0; kc < 4; ++kc) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      x[kc][i] = (bf16)(((float)x[kc][i] - mean) * inv * gs[32 * kc + g8 + i] + bs[32 * kc + g8 + i]);
  }
}

template <class T, int K, int TAPS, int NT, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void seqlin_d_kernel(SeqLinArgs a, int ntiles) {
  typedef Mfma<T> M;
  typedef typename M::frag F;
  constexpr int PAD = 16 / (int)sizeof(T), VEC = 16 / (int)sizeof(T), KS = K + PAD, NKC = K / M::KS;
  constexpr int NG = VEC / 4, IT = 16 * 16 * NT / VEC / 64;  // fp32 groups per chunk, chunks per lane (max)
  // the LDS epilogue only where its tile keeps two workgroups per CU (the 3-tap images take ~80 KB already)
  constexpr bool LE = TAPS == 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* Wt = (T*)smem;  // [TAPS * N][K + PAD]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), col = lane & 15, kof = M::koff(lane),
            g4 = 4 * (lane >> 4);
  const int ES = a.N + kSdEpad, cpr = a.N / VEC, nch = 16 * cpr;
  float* E = (float*)(Wt + TAPS * a.N * KS) + wave * 16 * ES;  // this wave's [16][N + pad] fp32 tile (LE)
  // LayerNorm parameters (LN form): after the image and the epilogue tiles
  float* Lg = (float*)(Wt + TAPS * a.N * KS) + (LE ? WAVES * 16 * ES : 0);
  constexpr bool LNF = sizeof(T) == 2 && K == 128;
  if constexpr (LNF)
    if (a.lng)
      for (int e = threadIdx.x; e < 2 * K; e += 64 * WAVES) Lg[e] = e < K ? a.lng[e] : a.lnb[e - K];
  // the bias, staged once (after the LayerNorm parameters' slots): the epilogue reads it from LDS (a global load
  // per output block, each used at once, was waited for in turn: NT round trips per tile)
  float* Lb = Lg + 2 * K;
  if (a.b)
    for (int e = threadIdx.x; e < a.N; e += 64 * WAVES) Lb[e] = a.b[e];
  constexpr int CPR = K / VEC;
  for (int e = threadIdx.x; e < TAPS * a.N * CPR; e += 64 * WAVES) {
    const int n = e / CPR, q = e % CPR;
    *(uint4*)(Wt + n * KS + q * VEC) = *(const uint4*)((const T*)a.wp + (size_t)n * K + q * VEC);
  }
  constexpr int kSdRows = 16 * WAVES;
  F bf[2][TAPS][NKC];
  uint4 rr[2][IT];      // LE: residual chunks of the lane's output chunks
  RawR4<T> r4[2][NT];   // otherwise: residual channels (4) of the lane's row per output tile
  // register double buffer: the slot is a compile-time constant (runtime-indexed register arrays spill)
  auto load_tile = [&](int tile, auto S) {
    constexpr int slot = decltype(S)::value;
    const int seq = tile / a.tiles_per_seq, tb = (tile - seq * a.tiles_per_seq) * kSdRows + wave * 16,
              t = tb + col;
#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap) {
      const int src = t + a.dir * (TAPS - 1 - tap);
      const bool ok = src >= 0 && src < a.T && t < a.T;
      const T* p = (const T*)a.x + ((long long)seq * a.T + (ok ? src : 0)) * a.ldx + kof;
#pragma unroll
      for (int kc = 0; kc < NKC; ++kc) {
        F v = M::load(p + kc * M::KS);
        if (!ok) v = F{};
        bf[slot][tap][kc] = v;
      }
    }
    if (a.r) {
      if constexpr (LE) {
#pragma unroll
        for (int i = 0; i < IT; ++i) {
          const int e = lane + 64 * i, row = e / cpr, q = e - row * cpr;
          if (e < nch && tb + row < a.T)
            rr[slot][i] = *(const uint4*)((const T*)a.r + ((long long)seq * a.T + tb + row) * a.ldr + q * VEC);
        }
      } else {
        const bool ok = t < a.T;
        const T* rp = (const T*)a.r + ((long long)seq * a.T + (ok ? t : 0)) * a.ldr + g4;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          if (nt * 16 < a.N) r4[slot][nt].v = *(const typename RawR4<T>::type*)(rp + nt * 16);
      }
    }
  };
  auto compute = [&](int tile, auto S) {
    constexpr int slot = decltype(S)::value;
    if constexpr (LNF) {
      if (a.lng) {  // normalise the rows now (their loads have landed); rows outside [0, T) stay zero
        const int seq = tile / a.tiles_per_seq, t = (tile - seq * a.tiles_per_seq) * kSdRows + wave * 16 + col;
#pragma unroll
        for (int tap = 0; tap < TAPS; ++tap) {
          const int src = t + a.dir * (TAPS - 1 - tap);
          ln_row_frags(bf[slot][tap], Lg, Lg + K, kof, a.lneps);
          if (!(src >= 0 && src < a.T && t < a.T))
#pragma unroll
            for (int kc = 0; kc < NKC; ++kc) bf[slot][tap][kc] = F{};
          __builtin_amdgcn_sched_barrier(0);  // one row set at a time (register pressure)
        }
      }
    }
    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap)
#pragma unroll
      for (int kc = 0; kc < NKC; ++kc) {
        const F b = bf[slot][tap][kc];
        const T* wb = Wt + (tap * a.N + col) * KS + kof + kc * M::KS;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          if (nt * 16 >= a.N) break;
          acc[nt] = M::mma(M::load(wb + nt * 16 * KS), b, acc[nt]);
        }
      }
    if constexpr (!LE) {  // lane (row = col, g): channels nt*16 + 4g .. +3 of its row straight to memory
      const int seq = tile / a.tiles_per_seq, t = (tile - seq * a.tiles_per_seq) * kSdRows + wave * 16 + col;
      if (t < a.T) {
        const long long row = (long long)seq * a.T + t;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          if (nt * 16 >= a.N) break;
          const int c = nt * 16 + g4;
          f32x4 v = acc[nt];
          if (a.b) v = v + *(const f32x4*)(Lb + c);
          if (a.r) v = v + r4[slot][nt].f();
          T* yp = (T*)a.y + row * a.ldy + c;
          if (a.accumulate) v = v + ld4((const T*)yp);
          st4(yp, v);
        }
      }
      return;
    }
    // lane (row = col, g) holds channels nt*16 + 4g .. +3 -> the wave's fp32 tile; LDS traffic of one wave
    // is processed in order, so its reads below see these writes
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      if (nt * 16 >= a.N) break;
      *(f32x4*)(E + col * ES + nt * 16 + g4) = acc[nt];
    }
    __builtin_amdgcn_wave_barrier();
    const int seq = tile / a.tiles_per_seq, tb = (tile - seq * a.tiles_per_seq) * kSdRows + wave * 16;
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int e = lane + 64 * i, row = e / cpr, q = e - row * cpr;
      if (e >= nch || tb + row >= a.T) continue;
      const long long grow = (long long)seq * a.T + tb + row;
      f32x4 v[NG], u[NG];
#pragma unroll
      for (int g = 0; g < NG; ++g) v[g] = *(const f32x4*)(E + row * ES + q * VEC + 4 * g);
      if (a.b)
#pragma unroll
        for (int g = 0; g < NG; ++g) v[g] = v[g] + *(const f32x4*)(Lb + q * VEC + 4 * g);
      if (a.r) {
        chunk_widen<T>(rr[slot][i], u);
#pragma unroll
        for (int g = 0; g < NG; ++g) v[g] = v[g] + u[g];
      }
      uint4* yp = (uint4*)((T*)a.y + grow * a.ldy + q * VEC);
      if (a.accumulate) {
        chunk_widen<T>(*yp, u);
#pragma unroll
        for (int g = 0; g < NG; ++g) v[g] = v[g] + u[g];
      }
      *yp = chunk_narrow<T>(v);
    }
    __builtin_amdgcn_wave_barrier();
  };
  typedef std::integral_constant<int, 0> S0;
  typedef std::integral_constant<int, 1> S1;
  const int G = gridDim.x;
  int tile = blockIdx.x;
  if (tile < ntiles) load_tile(tile, S0());
  __syncthreads();  // weight images staged
  for (; tile < ntiles; tile += 2 * G) {
    if (tile + G < ntiles) load_tile(tile + G, S1());
    compute(tile, S0());
    if (tile + G >= ntiles) break;
    if (tile + 2 * G < ntiles) load_tile(tile + 2 * G, S0());
    compute(tile + G, S1());
  }
}

// Weight preparation for seqlin: out[tap][n][k] = Wv[tap][k][n] in the activation dtype, for a batch of layers in
// one launch (blockIdx.y = descriptor). Run once per step; the forward passes and the data gradients then stage
// their weights with plain 16-byte copies.
constexpr int kMaxPrep = 48;
struct PrepBatch {
  vqa_seqlin_prep_desc d[kMaxPrep];
};

template <class T>
__global__ __launch_bounds__(256) void seqlin_prep_kernel(PrepBatch b) {
  const vqa_seqlin_prep_desc& d = b.d[blockIdx.y];
  const int total = d.taps * d.K * d.N;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
    const int tap = e / (d.N * d.K), rem = e - tap * d.N * d.K, n = rem / d.K, k = rem - n * d.K;
    const float v = d.wtrans ? d.w[((size_t)tap * d.N + n) * d.K + k] : d.w[((size_t)tap * d.K + k) * d.N + n];
    ((T*)d.out)[e] = (T)v;
  }
}

// Weight gradient of the sequence-linear layer (forward direction dir = -1 or taps = 1):
//   dW[tap][k][n] = sum_t X[t - (taps-1-tap)][k] dY[t][n],  db[n] = sum_t dY[t][n]
// Workgroup = one row segment of one sequence, 64-row chunks staged in LDS; MFMA K = rows via transposed
// fragment reads (Mfma::rows). Wave w owns the (tap, k-tile) pairs p = w, w+4, ... and every n-tile: per
// 32-row step it reads NT dY fragments and one X fragment per pair. One fp32 partial row per workgroup:
// [dW (taps*K*N) | db (N)].
struct SeqWgArgs {
  const void* x;
  const void* dy;
  float* part;
  long long ldx, lddy;
  int nseq, T, K, N, taps, seg_rows, segs_per_seq;
};

template <class T, int PPW, int NT>
__global__ __launch_bounds__(256) void seqlin_wgrad_kernel(SeqWgArgs a) {
  typedef Mfma<T> M;
  constexpr int PAD = 16 / (int)sizeof(T), CH = 64;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int XS = a.K + PAD, YS = a.N + PAD, halo = a.taps - 1;
  T* X = (T*)smem;               // [CH + halo][K + PAD]; row j <-> time c0 - halo + j
  T* Y = X + (CH + halo) * XS;   // [CH][N + PAD]
  const int seq = blockIdx.x / a.segs_per_seq, seg = blockIdx.x - seq * a.segs_per_seq;
  const int tb = seg * a.seg_rows, te = std::min(a.T, tb + a.seg_rows);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int npairs = a.taps * (a.K / 16);
  f32x4 acc[PPW][NT], accb[NT];
#pragma unroll
  for (int p = 0; p < PPW; ++p)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[p][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) accb[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool bias_wave = wave == 3;  // the wave with the fewest pairs also sums the bias
  constexpr int VEC = 16 / (int)sizeof(T);
  for (int c0 = tb; c0 < te; c0 += CH) {
    __syncthreads();
    const int cx = a.K / VEC, cy = a.N / VEC;
    for (int e = threadIdx.x; e < (CH + halo) * cx; e += 256) {
      const int j = e / cx, q = e - j * cx, t = c0 - halo + j;
      uint4 v = {0u, 0u, 0u, 0u};
      // source rows of this segment's outputs only: t < te (rows past the segment belong to the next one)
      if (t >= 0 && t < te) v = *(const uint4*)((const T*)a.x + ((long long)seq * a.T + t) * a.ldx + q * VEC);
      *(uint4*)(X + j * XS + q * VEC) = v;
    }
    for (int e = threadIdx.x; e < CH * cy; e += 256) {
      const int j = e / cy, q = e - j * cy, t = c0 + j;
      uint4 v = {0u, 0u, 0u, 0u};
      if (t < te) v = *(const uint4*)((const T*)a.dy + ((long long)seq * a.T + t) * a.lddy + q * VEC);
      *(uint4*)(Y + j * YS + q * VEC) = v;
    }
    __syncthreads();
    for (int kk = 0; kk < CH; kk += M::KS) {
      typename M::frag bf[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) bf[nt] = nt * 16 < a.N ? M::rows(Y + kk * YS + nt * 16, YS) : bf[0];
#pragma unroll
      for (int p = 0; p < PPW; ++p) {
        const int pr = wave + 4 * p;
        if (pr >= npairs) break;
        const int tap = pr / (a.K / 16), kt = pr - tap * (a.K / 16);
        const typename M::frag af = M::rows(X + (kk + tap) * XS + kt * 16, XS);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          if (nt * 16 < a.N) acc[p][nt] = M::mma(af, bf[nt], acc[p][nt]);
      }
      if (bias_wave) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          if (nt * 16 < a.N) accb[nt] = M::mma(M::ones(), bf[nt], accb[nt]);
      }
    }
  }
  float* part = a.part + (size_t)blockIdx.x * ((size_t)a.taps * a.K * a.N + a.N);
  const int n = lane & 15, g4 = 4 * (lane >> 4);
#pragma unroll
  for (int p = 0; p < PPW; ++p) {
    const int pr = wave + 4 * p;
    if (pr >= npairs) break;
    const int tap = pr / (a.K / 16), kt = pr - tap * (a.K / 16);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      if (nt * 16 >= a.N) break;
#pragma unroll
      for (int i = 0; i < 4; ++i) part[((size_t)tap * a.K + kt * 16 + g4 + i) * a.N + nt * 16 + n] = acc[p][nt][i];
    }
  }
  if (bias_wave && lane < 16) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      if (nt * 16 < a.N) part[(size_t)a.taps * a.K * a.N + nt * 16 + n] = accb[nt][0];
  }
}

// ---------------------------------------------------------------------------------------------------
static size_t seqlin_lds(int K, int N, int taps, int esz) {
  const int ks = K + 16 / esz;
  return ((size_t)N * ks + (size_t)(kSlRows + taps - 1) * ks) * esz;
}
static size_t wgrad_lds(int K, int N, int taps, int esz) {
  return ((size_t)(64 + taps - 1) * (K + 16 / esz) + (size_t)64 * (N + 16 / esz)) * esz;
}

// The (K, taps) pairs seqlin_d_kernel is instantiated for
#define VQA_SD_SHAPES(X) X(32, 1) X(128, 1) X(96, 3) X(128, 3)

// What a sequence-linear call runs, settled on the host from the arguments alone (vqa_seqlin_route reports it; the
// launch below follows it): the persistent direct form (a prepared image of every tap in LDS) or the staged form
// (one tap's weights in LDS at a time, from raw fp32 weights or a prepared image), with its geometry.
struct SeqlinPlan {
  int direct, waves, tile_rows, workgroups, tiles, nt;
  size_t lds;
};

static int seqlin_plan(const SeqLinArgs& a, int esz, SeqlinPlan& p) {
  constexpr size_t kLdsMax = 160 * 1024;
  if (a.wp) {
    // wide outputs: 8 waves per workgroup share one staged weight image (one workgroup per CU); narrow ones:
    // 4 waves, two workgroups per CU (measured per shape, tools/seqlin_time.py)
    const bool n2 = a.N <= 32, w8 = a.N >= 96;
    const int waves = w8 ? 8 : 4, max_per_cu = w8 ? 1 : 2;
    const int KS = a.K + 16 / esz;
    const size_t lds = (size_t)a.taps * a.N * KS * esz +
                       (a.taps == 1 ? (size_t)waves * 16 * (a.N + kSdEpad) * sizeof(float) : 0) +
                       (size_t)(2 * a.K + a.N) * sizeof(float);  // LayerNorm slots (used or not) + the bias
    bool inst = false;
#define VQA_SD(KK, TT) inst = inst || (a.K == KK && a.taps == TT);
    VQA_SD_SHAPES(VQA_SD)
#undef VQA_SD
    // the 1-tap epilogue stores (and reads the residual) in whole 16-byte chunks
    const int vec = 16 / esz;
    const bool chunks = a.taps != 1 || (a.ldy % vec == 0 && ((uintptr_t)a.y & 15) == 0 &&
                                        (!a.r || (a.ldr % vec == 0 && ((uintptr_t)a.r & 15) == 0)));
    if (inst && chunks && lds <= kLdsMax) {
      const int tps = (a.T + 16 * waves - 1) / (16 * waves), ntiles = a.nseq * tps;
      const int per_cu = std::max(1, std::min<int>(max_per_cu, (int)(kLdsMax / lds)));
      p = SeqlinPlan{1, waves, 16 * waves, std::min(ntiles, cu_count() * per_cu), ntiles, n2 ? 2 : 8, lds};
      return VQA_OK;
    }
    // weights too large for one LDS image (or no direct instantiation, or unaligned 1-tap rows): stage per tap
    // from the prepared image
  }
  VQA_REQUIRE(!a.lng, VQA_E_UNSUPPORTED, "seqlin_fwd_ln_prepped: K=%d N=%d taps=%d has no fused form", a.K, a.N,
              a.taps);
  const size_t lds = seqlin_lds(a.K, a.N, a.taps, esz);
  VQA_REQUIRE(lds <= kLdsMax, VQA_E_UNSUPPORTED,
              "seqlin_fwd: K=%d N=%d taps=%d needs %zu bytes of LDS for its tiles (limit %zu)", a.K, a.N, a.taps, lds,
              kLdsMax);
  const int ntiles = a.nseq * ((a.T + kSlRows - 1) / kSlRows);
  p = SeqlinPlan{0, 4, kSlRows, ntiles, ntiles, a.N <= 32 ? 2 : 8, lds};
  return VQA_OK;
}

template <class T>
static int launch_seqlin(const SeqLinArgs& a, hipStream_t s) {
  SeqlinPlan p;
  if (int rc = seqlin_plan(a, (int)sizeof(T), p)) return rc;
  SeqLinArgs c = a;
  if (p.direct) {
    const void* fn = nullptr;
#define VQA_SD(KK, TT)                                                                                         \
    if (a.K == KK && a.taps == TT)                                                                           \
      fn = p.nt == 2 ? (const void*)seqlin_d_kernel<T, KK, TT, 2, 4>                                         \
                     : p.waves == 8 ? (const void*)seqlin_d_kernel<T, KK, TT, 8, 8>                          \
                                    : (const void*)seqlin_d_kernel<T, KK, TT, 8, 4>;
    VQA_SD_SHAPES(VQA_SD)
#undef VQA_SD
    VQA_REQUIRE(fn, VQA_E_UNSUPPORTED, "seqlin_fwd: no direct kernel for K=%d taps=%d", a.K, a.taps);
    if (int rc = raise_dyn_lds(fn, p.lds, "prior")) return rc;
    c.tiles_per_seq = (a.T + p.tile_rows - 1) / p.tile_rows;
    int ntiles = p.tiles;
    void* args[] = {&c, &ntiles};
    (void)hipLaunchKernel(fn, dim3(p.workgroups), dim3(64 * p.waves), args, p.lds, s);
    VQA_LAUNCHED("seqlin_d_kernel");
    return VQA_OK;
  }
  const void* fn = p.nt == 2 ? (const void*)seqlin_kernel<T, 2> : (const void*)seqlin_kernel<T, 8>;
  if (int rc = raise_dyn_lds(fn, p.lds, "prior")) return rc;
  void* args[] = {&c};
  (void)hipLaunchKernel(fn, dim3(p.workgroups), dim3(256), args, p.lds, s);
  VQA_LAUNCHED("seqlin_kernel");
  return VQA_OK;
}

template <class T>
static const void* wgrad_fn(int ppw, int N) {
  const bool n2 = N <= 32;
  if (ppw <= 1) return n2 ? (const void*)seqlin_wgrad_kernel<T, 1, 2> : (const void*)seqlin_wgrad_kernel<T, 1, 8>;
  if (ppw <= 2) return n2 ? (const void*)seqlin_wgrad_kernel<T, 2, 2> : (const void*)seqlin_wgrad_kernel<T, 2, 8>;
  return n2 ? (const void*)seqlin_wgrad_kernel<T, 6, 2> : (const void*)seqlin_wgrad_kernel<T, 6, 8>;
}

static void wgrad_plan(int nseq, int T, int& seg_rows, int& segs) {
  // about 2 workgroups per CU in total, segments a multiple of the 64-row chunk
  const long long target = std::max<long long>(1, (long long)2 * cu_count() / std::max(1, nseq));
  seg_rows = (int)std::max<long long>(64, ((T + target - 1) / target + 63) / 64 * 64);
  segs = (T + seg_rows - 1) / seg_rows;
}

}  // namespace vqa

using namespace vqa;

extern "C" int vqa_seqlin_prep(const vqa_seqlin_prep_desc* descs, int count, int dtype, vqa_stream_t stream) {
  VQA_ARG(descs && count > 0 && pr_dt(dtype), "seqlin_prep: bad arguments");
  for (int i0 = 0; i0 < count; i0 += kMaxPrep) {
    PrepBatch b;
    const int n = std::min(kMaxPrep, count - i0);
    for (int i = 0; i < n; ++i) {
      b.d[i] = descs[i0 + i];
      VQA_ARG(b.d[i].w && b.d[i].out && b.d[i].taps > 0 && b.d[i].K > 0 && b.d[i].N > 0, "seqlin_prep: descriptor %d",
              i0 + i);
    }
    if (dtype == VQA_BF16)
      hipLaunchKernelGGL(seqlin_prep_kernel<bf16>, dim3(16, n), dim3(256), 0, (hipStream_t)stream, b);
    else
      hipLaunchKernelGGL(seqlin_prep_kernel<float>, dim3(16, n), dim3(256), 0, (hipStream_t)stream, b);
    VQA_LAUNCHED("seqlin_prep_kernel");
  }
  return VQA_OK;
}

// argument checks of every sequence-linear entry point (host only) -> the kernels' argument block
static int seqlin_args(const void* x, int64_t ldx, const float* w, const void* wp, const float* bias,
                       const void* residual, int64_t ldr, void* y, int64_t ldy, int nseq, int T, int K, int N,
                       int taps, int dir, int wtrans, int accumulate, int dtype, SeqLinArgs& a) {
  VQA_ARG(x && (w || wp) && y && nseq > 0 && T > 0 && (taps == 1 || taps == 3) && (dir == -1 || dir == 1),
          "seqlin_fwd: bad arguments");
  VQA_ARG(pr_dt(dtype), "seqlin_fwd: unknown dtype %d", dtype);
  const int esz = dtype == VQA_BF16 ? 2 : 4, vec = 16 / esz;
  VQA_REQUIRE(K > 0 && K <= 256 && K % (dtype == VQA_BF16 ? 32 : 4) == 0 && N > 0 && N <= 128 && N % 16 == 0,
              VQA_E_UNSUPPORTED, "seqlin_fwd: K=%d N=%d unsupported", K, N);
  VQA_ARG(ldx % vec == 0 && ldy % 4 == 0 && (!residual || ldr % 4 == 0) && ldx >= K && ldy >= N,
          "seqlin_fwd: strides must keep 16-byte rows");
  VQA_ARG(((uintptr_t)(w ? (const void*)w : wp) & 15) == 0, "seqlin_fwd: weights must be 16-byte aligned");
  a = SeqLinArgs{x, w, wp, bias, residual, y, ldx, ldr, ldy, nseq, T, K, N, taps, dir, wtrans, accumulate,
                 (T + kSlRows - 1) / kSlRows};
  return VQA_OK;
}

static int seqlin_ln_args(const void* x, int64_t ldx, const float* gamma, const float* beta, float eps, const void* wp,
                          const float* bias, const void* residual, int64_t ldr, void* y, int64_t ldy, int nseq, int T,
                          int K, int N, int taps, int dir, int dtype, SeqLinArgs& a) {
  VQA_ARG(x && wp && y && gamma && beta && nseq > 0 && T > 0 && (taps == 1 || taps == 3) && (dir == -1 || dir == 1),
          "seqlin_fwd_ln_prepped: bad arguments");
  VQA_REQUIRE(dtype == VQA_BF16 && K == 128 && N > 0 && N <= 128 && N % 16 == 0, VQA_E_UNSUPPORTED,
              "seqlin_fwd_ln_prepped: dtype %d K=%d N=%d unsupported (bf16, K = 128)", dtype, K, N);
  VQA_ARG(ldx % 8 == 0 && ldx >= K && ldy >= N && ldy % 4 == 0 && (!residual || ldr % 4 == 0),
          "seqlin_fwd_ln_prepped: strides must keep 16-byte rows");
  VQA_ARG(((uintptr_t)wp & 15) == 0, "seqlin_fwd_ln_prepped: weights must be 16-byte aligned");
  a = SeqLinArgs{x, nullptr, wp, bias, residual, y, ldx, ldr, ldy, nseq, T, K, N, taps, dir, 0, 0,
                 (T + kSlRows - 1) / kSlRows, gamma, beta, eps};
  return VQA_OK;
}

static int seqlin_launch(const void* x, int64_t ldx, const float* w, const void* wp, const float* bias,
                         const void* residual, int64_t ldr, void* y, int64_t ldy, int nseq, int T, int K, int N,
                         int taps, int dir, int wtrans, int accumulate, int dtype, hipStream_t s) {
  SeqLinArgs a;
  if (int rc = seqlin_args(x, ldx, w, wp, bias, residual, ldr, y, ldy, nseq, T, K, N, taps, dir, wtrans, accumulate,
                           dtype, a))
    return rc;
  return dtype == VQA_BF16 ? launch_seqlin<bf16>(a, s) : launch_seqlin<float>(a, s);
}

extern "C" int vqa_seqlin_route(const void* x, int64_t ldx, const float* w, const void* wp, const float* bias,
                                const void* residual, int64_t ldr, void* y, int64_t ldy, int nseq, int T, int K, int N,
                                int taps, int dir, int wtrans, int accumulate, int dtype, int layernorm,
                                vqa_seqlin_route_info* route) {
  VQA_ARG(route, "seqlin_route: null route");
  SeqLinArgs a;
  if (layernorm) {
    // the fused form's LayerNorm parameters are only tested for presence: stand-ins that are never read
    static const float one = 1.f;
    if (int rc = seqlin_ln_args(x, ldx, &one, &one, 0.f, wp, bias, residual, ldr, y, ldy, nseq, T, K, N, taps, dir,
                                dtype, a))
      return rc;
  } else if (int rc = seqlin_args(x, ldx, w, wp, bias, residual, ldr, y, ldy, nseq, T, K, N, taps, dir, wtrans,
                                  accumulate, dtype, a)) {
    return rc;
  }
  SeqlinPlan p;
  if (int rc = seqlin_plan(a, dtype == VQA_BF16 ? 2 : 4, p)) return rc;
  *route = vqa_seqlin_route_info{p.direct, p.waves, p.tile_rows, p.workgroups, p.tiles, p.nt, (int64_t)p.lds};
  return VQA_OK;
}

extern "C" int vqa_seqlin_fwd(const void* x, int64_t ldx, const float* w, const float* bias, const void* residual,
                              int64_t ldr, void* y, int64_t ldy, int nseq, int T, int K, int N, int taps, int dir,
                              int wtrans, int accumulate, int dtype, vqa_stream_t stream) {
  VQA_ARG(w, "seqlin_fwd: no weights");
  return seqlin_launch(x, ldx, w, nullptr, bias, residual, ldr, y, ldy, nseq, T, K, N, taps, dir, wtrans, accumulate,
                       dtype, (hipStream_t)stream);
}

extern "C" int vqa_seqlin_fwd_prepped(const void* x, int64_t ldx, const void* wp, const float* bias,
                                      const void* residual, int64_t ldr, void* y, int64_t ldy, int nseq, int T, int K,
                                      int N, int taps, int dir, int accumulate, int dtype, vqa_stream_t stream) {
  VQA_ARG(wp, "seqlin_fwd_prepped: no weights");
  return seqlin_launch(x, ldx, nullptr, wp, bias, residual, ldr, y, ldy, nseq, T, K, N, taps, dir, 0, accumulate,
                       dtype, (hipStream_t)stream);
}

extern "C" int vqa_seqlin_fwd_ln_prepped(const void* x, int64_t ldx, const float* gamma, const float* beta,
                                         float eps, const void* wp, const float* bias, const void* residual,
                                         int64_t ldr, void* y, int64_t ldy, int nseq, int T, int K, int N, int taps,
                                         int dir, int dtype, vqa_stream_t stream) {
  SeqLinArgs a;
  if (int rc = seqlin_ln_args(x, ldx, gamma, beta, eps, wp, bias, residual, ldr, y, ldy, nseq, T, K, N, taps, dir,
                              dtype, a))
    return rc;
  return launch_seqlin<bf16>(a, (hipStream_t)stream);
}

extern "C" size_t vqa_seqlin_wgrad_workspace(int nseq, int T, int K, int N, int taps) {
  if (nseq < 1 || T < 1 || K < 1 || N < 1 || taps < 1) return 0;
  int seg_rows, segs;
  wgrad_plan(nseq, T, seg_rows, segs);
  return (size_t)nseq * segs * ((size_t)taps * K * N + N) * sizeof(float);
}

// shape checks and launch geometry of vqa_seqlin_wgrad (host only; vqa_seqlin_wgrad_plan reports them)
static int wgrad_route(int nseq, int T, int K, int N, int taps, int dtype, int& seg_rows, int& segs, int& ppw) {
  VQA_ARG(nseq > 0 && T > 0 && (taps == 1 || taps == 3), "seqlin_wgrad: bad arguments");
  VQA_ARG(pr_dt(dtype), "seqlin_wgrad: unknown dtype %d", dtype);
  VQA_REQUIRE(K > 0 && K % 16 == 0 && K <= 128 && N > 0 && N % 16 == 0 && N <= 128 && (taps * K / 16 + 3) / 4 <= 6,
              VQA_E_UNSUPPORTED, "seqlin_wgrad: K=%d N=%d taps=%d unsupported", K, N, taps);
  wgrad_plan(nseq, T, seg_rows, segs);
  const int need = (taps * K / 16 + 3) / 4;  // (tap, k-tile) pairs of the busiest wave
  ppw = need <= 1 ? 1 : need <= 2 ? 2 : 6;   // the instantiations of seqlin_wgrad_kernel
  return VQA_OK;
}

extern "C" int vqa_seqlin_wgrad_plan(int nseq, int T, int K, int N, int taps, int dtype, int* seg_rows, int* segs,
                                     int* pairs_per_wave) {
  VQA_ARG(seg_rows && segs && pairs_per_wave, "seqlin_wgrad_plan: null seg_rows, segs or pairs_per_wave");
  int sr, sg, ppw;
  if (int rc = wgrad_route(nseq, T, K, N, taps, dtype, sr, sg, ppw)) return rc;
  *seg_rows = sr;
  *segs = sg;
  *pairs_per_wave = ppw;
  return VQA_OK;
}

extern "C" int vqa_seqlin_wgrad(const void* x, int64_t ldx, const void* dy, int64_t lddy, float* dw, float* db,
                                int nseq, int T, int K, int N, int taps, int dtype, void* workspace, size_t ws_bytes,
                                vqa_partials_desc* desc, vqa_stream_t stream) {
  VQA_ARG(x && dy && dw, "seqlin_wgrad: bad arguments");
  int seg_rows, segs, ppw;
  if (int rc = wgrad_route(nseq, T, K, N, taps, dtype, seg_rows, segs, ppw)) return rc;
  const int esz = dtype == VQA_BF16 ? 2 : 4, vec = 16 / esz;
  VQA_ARG(ldx % vec == 0 && lddy % vec == 0, "seqlin_wgrad: strides must keep 16-byte rows");
  const size_t need = vqa_seqlin_wgrad_workspace(nseq, T, K, N, taps);
  VQA_ARG(workspace && ws_bytes >= need, "seqlin_wgrad: workspace %zu < %zu", ws_bytes, need);
  SeqWgArgs a{x, dy, (float*)workspace, ldx, lddy, nseq, T, K, N, taps, seg_rows, segs};
  const void* fn = dtype == VQA_BF16 ? wgrad_fn<bf16>(ppw, N) : wgrad_fn<float>(ppw, N);
  const size_t lds = wgrad_lds(K, N, taps, esz);
  if (int rc = raise_dyn_lds(fn, lds, "prior")) return rc;
  void* args[] = {&a};
  (void)hipLaunchKernel(fn, dim3(nseq * segs), dim3(256), args, lds, (hipStream_t)stream);
  VQA_LAUNCHED("seqlin_wgrad_kernel");
  const int E = taps * K * N + N;
  const vqa_partials_desc d{(const float*)workspace, dw, db, nseq * segs, E, taps * K * N, 0};
  if (desc) {
    *desc = d;
    return VQA_OK;
  }
  return vqa_reduce_partials(&d, 1, stream);
}
