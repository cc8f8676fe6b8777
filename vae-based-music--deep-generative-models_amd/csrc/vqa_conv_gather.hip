// vqa_conv_gather.hip — the gather convolution kernels (forward and data gradient of every conv and transposed
// conv; vqa_conv.h has the formulation), the host plan of each and the one routing list run_gather launches from.
#include "vqa_conv.h"
#include "vqa_launch.h"
#include "vqa_mfma.h"
#include <algorithm>

namespace vqa {

// ------------------------------------------------------------------------------------------------
// Generic VALU gather conv: any C/O/K/S/D, mixed fp32/bf16 ends. Used for the 1-channel layers at
// the waveform ends (first encoder conv C=1, decoder output conv O=1 and its data-gradient), and as the
// fall-through for 32- / 64-channel tiles too large for the MFMA kernel's stager or LDS. Such a bf16 conv takes
// its weights rounded to bf16 (a.wbf16), as the MFMA kernels stage them: which of the two kernels it runs depends
// on its epilogue flags, and its result must not (bf16 x bf16 products are exact in fp32; only the order of the
// fp32 sum differs).

template <class TX, class TY>
__global__ __launch_bounds__(256) void gather_direct_kernel(GatherArgs a) {
  const TX* X = (const TX*)a.x;
  const long long total = (long long)a.B * a.T_out * a.O;
  const bool relu = a.flags & VQA_PRE_RELU;
  const bool wb = a.wbf16;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const int o = (int)(e % a.O);
    const long long r = e / a.O;
    const int t = (int)(r % a.T_out);
    const int n = (int)(r / a.T_out);
    float acc = 0.f;
    for (int k = 0; k < a.K; ++k) {
      const int ti = t * a.S + k * a.D - a.P;
      if (ti < 0 || ti >= a.T_in) continue;
      const TX* xr = X + ((long long)n * a.T_in + ti) * a.C;
      for (int c = 0; c < a.C; ++c) {
        float xv = ld(xr + c);
        if (relu) xv = fmaxf(xv, 0.f);
        const float w = weff(a, k, c, o);
        acc += xv * (wb ? (float)(bf16)w : w);
      }
    }
    const long long oi = out_index(a, n, t, o);
    if (oi < 0) continue;
    float v = acc;
    if (a.bias) v = v + a.bias[bias_index(a, o)];
    if (a.flags & VQA_POST_MASK) v = ld((const TY*)a.mask + oi) > 0.f ? v : 0.f;
    if (a.flags & VQA_ADD_RESIDUAL) v = ld((const TY*)a.resid + oi) + v;
    st((TY*)a.y + oi, v);
  }
}

// ------------------------------------------------------------------------------------------------
// Thin gather conv for the 1-channel waveform layers (C <= 8 or O <= 8): weights in LDS (fp32), each
// thread owns OV consecutive output channels of one row; 16-byte loads along C when C % 8 == 0.
template <class TX, class TY, int OV>
__global__ __launch_bounds__(256) void gather_thin_kernel(GatherArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* wl = (float*)smem;  // [K][C][O]
  const int KCO = a.K * a.C * a.O;
  for (int e = threadIdx.x; e < KCO; e += blockDim.x) {
    const int o = e % a.O, c = (e / a.O) % a.C, k = e / (a.O * a.C);
    wl[e] = weff(a, k, c, o);
  }
  __syncthreads();
  const TX* X = (const TX*)a.x;
  const int OG = a.O / OV;
  const int total = a.B * a.T_out * OG;  // < 2^31 (host-checked)
  const bool relu = a.flags & VQA_PRE_RELU;
  const bool vec = (a.C % 8) == 0;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const int og = e % OG;
    const int r = e / OG;
    const int t = r % a.T_out;
    const int n = r / a.T_out;
    float acc[OV];
#pragma unroll
    for (int q = 0; q < OV; ++q) acc[q] = 0.f;
    for (int k = 0; k < a.K; ++k) {
      const int ti = t * a.S + k * a.D - a.P;
      if (ti < 0 || ti >= a.T_in) continue;
      const TX* xr = X + ((long long)n * a.T_in + ti) * a.C;
      const float* wk = wl + (size_t)k * a.C * a.O + og * OV;
      if (vec) {
        for (int c0 = 0; c0 < a.C; c0 += 8) {
          float xv[8];
          ld8(xr + c0, xv);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float xj = relu ? fmaxf(xv[j], 0.f) : xv[j];
#pragma unroll
            for (int q = 0; q < OV; ++q) acc[q] += xj * wk[(c0 + j) * a.O + q];
          }
        }
      } else {
        for (int c = 0; c < a.C; ++c) {
          float xs = ld(xr + c);
          if (relu) xs = fmaxf(xs, 0.f);
#pragma unroll
          for (int q = 0; q < OV; ++q) acc[q] += xs * wk[c * a.O + q];
        }
      }
    }
    const int o0 = og * OV;
    const long long oi = out_index(a, n, t, o0);
    if (oi < 0) continue;
    const int bo = bias_index(a, o0);
    if constexpr (OV == 8) {
      if (a.O % 16 == 0) {  // the 8 channels are contiguous and 16-byte aligned in every mode: one vector access
        float v[8], m[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = a.bias ? acc[q] + a.bias[bo + q] : acc[q];
        if (a.flags & VQA_POST_MASK) {
          ld8((const TY*)a.mask + oi, m);
#pragma unroll
          for (int q = 0; q < 8; ++q) v[q] = m[q] > 0.f ? v[q] : 0.f;
        }
        if (a.flags & VQA_ADD_RESIDUAL) {
          ld8((const TY*)a.resid + oi, m);
#pragma unroll
          for (int q = 0; q < 8; ++q) v[q] = m[q] + v[q];
        }
        st8((TY*)a.y + oi, v);
        continue;
      }
    }
#pragma unroll
    for (int q = 0; q < OV; ++q) {
      float v = acc[q];
      if (a.bias) v = v + a.bias[bo + q];
      if (a.flags & VQA_POST_MASK) v = ld((const TY*)a.mask + oi + q) > 0.f ? v : 0.f;
      if (a.flags & VQA_ADD_RESIDUAL) v = ld((const TY*)a.resid + oi + q) + v;
      st((TY*)a.y + oi + q, v);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Stage rows [r0, r0+rows) of one item (Xi = that item's row 0, channels C) into LDS with padded row
// stride XS, zero-filling rows outside [lo, hi), optional ReLU. 16-byte vector loads.
template <class T, int C>
__device__ __forceinline__ void stage_rows(T* xl, int XS, const T* Xi, int lo, int hi, int r0, int rows,
                                           bool relu) {
  constexpr int VEC = 16 / (int)sizeof(T);
  constexpr int CPR = C / VEC;
  for (int e = threadIdx.x; e < rows * CPR; e += blockDim.x) {
    const int rr = e / CPR, q = e - rr * CPR;
    const int ti = r0 + rr;
    uint4 v = {0u, 0u, 0u, 0u};
    if (ti >= lo && ti < hi) v = *((const uint4*)(Xi + (long long)ti * C) + q);
    if (relu) relu_bits<T>(v);
    *(uint4*)(xl + rr * XS + q * VEC) = v;
  }
}

// Narrow-output gather conv (O <= 8, C in {32, 64}; the decoder output conv C=64 -> O=1): one block =
// TB output rows of one item; the input rows are staged through LDS with coalesced 16-byte loads and
// every thread reduces one output row from LDS.
template <class TX, class TY, int C>
__global__ __launch_bounds__(256) void gather_thinO_kernel(GatherArgs a, int ntb) {
  constexpr int TB = 256;
  constexpr int XS = C + 16 / (int)sizeof(TX);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* wl = (float*)smem;  // [K][C][O]
  const int KCO = a.K * C * a.O;
  TX* xl = (TX*)(smem + ((KCO * 4 + 15) / 16) * 16);
  const int n = blockIdx.x / ntb, t0 = (blockIdx.x - n * ntb) * TB;
  for (int e = threadIdx.x; e < KCO; e += 256) {
    const int o = e % a.O, c = (e / a.O) % C, k = e / (a.O * C);
    wl[e] = weff(a, k, c, o);
  }
  const int rows_in = (TB - 1) * a.S + (a.K - 1) * a.D + 1;
  stage_rows<TX, C>(xl, XS, (const TX*)a.x + (long long)n * a.T_in * C, 0, a.T_in, t0 * a.S - a.P, rows_in,
                    a.flags & VQA_PRE_RELU);
  __syncthreads();
  const int t = t0 + threadIdx.x;
  if (t >= a.T_out) return;
  float acc[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) acc[o] = 0.f;
  for (int k = 0; k < a.K; ++k) {
    const TX* xr = xl + (threadIdx.x * a.S + k * a.D) * XS;
    const float* wk = wl + k * C * a.O;
#pragma unroll
    for (int c0 = 0; c0 < C; c0 += 8) {
      float xv[8];
      ld8(xr + c0, xv);
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int o = 0; o < 8; ++o)
          if (o < a.O) acc[o] += xv[j] * wk[(c0 + j) * a.O + o];
    }
  }
  const long long oi = out_index(a, n, t, 0);
#pragma unroll
  for (int o = 0; o < 8; ++o) {
    if (o < a.O) {
      float v = acc[o];
      if (a.bias) v = v + a.bias[o];
      if (a.flags & VQA_POST_MASK) v = ld((const TY*)a.mask + oi + o) > 0.f ? v : 0.f;
      if (a.flags & VQA_ADD_RESIDUAL) v = ld((const TY*)a.resid + oi + o) + v;
      st((TY*)a.y + oi + o, v);
    }
  }
}

// Weights -> LDS image [K][O][C + pad] in T: 16-byte loads along the Keras kernel's contiguous axis, every
// load of a batch issued before any store. DIRECT (w[k][c][o]: o contiguous) moves (tap, input-channel pair,
// output quad) items — two float4 loads, four packed-pair stores; FLIP_T / PAIR (c contiguous) move (tap,
// output channel, input quad) items — one float4 load, one 4-element store. (The per-element form — a scalar
// load and a 2-byte store per weight — took ~5 us at the start of every workgroup: 0.41 ms of the step's
// 1.98 ms of conv time, tools/conv_sweep.py.)
template <class T> __device__ __forceinline__ void st2w(T* p, float a, float b);
template <> __device__ __forceinline__ void st2w<float>(float* p, float a, float b) {
  typedef float f2 __attribute__((ext_vector_type(2)));
  *(f2*)p = f2{a, b};
}
template <> __device__ __forceinline__ void st2w<bf16>(bf16* p, float a, float b) {
  typedef float f2 __attribute__((ext_vector_type(2)));
  typedef __bf16 b2 __attribute__((ext_vector_type(2)));
  *(b2*)p = __builtin_convertvector((f2){a, b}, b2);
}

template <class T, int C, int O>
__device__ __forceinline__ void stage_weights(const GatherArgs& a, T* wl, int WS) {
  static_assert(C % 4 == 0 && O % 4 == 0, "vector weight staging");
  constexpr int NB = 4;  // items in flight per thread
  if (a.wmode == W_DIRECT) {
    constexpr int OQ = O / 4, CP = C / 2;
    const int items = a.K * CP * OQ;
    for (int e0 = 0; e0 < items; e0 += 256 * NB) {
      f32x4 lo[NB], hi[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int e = e0 + threadIdx.x + j * 256;
        lo[j] = hi[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (e < items) {
          const int oq = e % OQ, cp = (e / OQ) % CP, k = e / (OQ * CP);
          const float* src = a.w + ((size_t)k * C + 2 * cp) * O + 4 * oq;
          lo[j] = *(const f32x4*)src;
          hi[j] = *(const f32x4*)(src + O);
        }
      }
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int e = e0 + threadIdx.x + j * 256;
        if (e < items) {
          const int oq = e % OQ, cp = (e / OQ) % CP, k = e / (OQ * CP);
          T* dst = wl + ((size_t)k * O + 4 * oq) * WS + 2 * cp;
#pragma unroll
          for (int i = 0; i < 4; ++i) st2w<T>(dst + i * WS, lo[j][i], hi[j][i]);
        }
      }
    }
  } else {
    constexpr int CQ = C / 4;
    const int items = a.K * O * CQ;
    for (int e0 = 0; e0 < items; e0 += 256 * NB) {
      f32x4 v[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int e = e0 + threadIdx.x + j * 256;
        v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (e < items) {
          const int cq = e % CQ, o = (e / CQ) % O, k = e / (CQ * O);
          const float* src = nullptr;
          if (a.wmode == W_FLIP_T) {
            src = a.w + ((size_t)(a.Kb - 1 - k) * O + o) * C + 4 * cq;
          } else {  // PAIR: out pair column o = (p, ob) takes base tap kb = p + Pb - 2 (k - 1), zero outside
            const int Ob = O >> 1, p = o >= Ob ? 1 : 0, ob = o - p * Ob, kb = p + a.Pb - 2 * (k - 1);
            if (kb >= 0 && kb < a.Kb) src = a.w + ((size_t)kb * Ob + ob) * C + 4 * cq;
          }
          if (src) v[j] = *(const f32x4*)src;
        }
      }
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int e = e0 + threadIdx.x + j * 256;
        if (e < items) {
          const int cq = e % CQ, o = (e / CQ) % O, k = e / (CQ * O);
          st4<T>(wl + ((size_t)k * O + o) * WS + 4 * cq, v[j]);
        }
      }
    }
  }
}

// One tile's global -> LDS copy in 16-byte chunks, held in registers between load() and store():
// chunks [0, nx) are the input rows (with halo; padded LDS rows, compile-time chunks per row), then ne
// chunks of the ReLU' mask and ne of the residual — the output rows of the tile, contiguous in global
// memory, copied chunk-linearly (unpadded) into their LDS tiles. Chunk e = threadIdx.x + i*256.
struct TileSrc {
  const char* x;      // this item's input row 0
  int r0, nx;         // first input row of the tile, input chunks
  const char* m;      // mask bytes of the tile's first output row (nullptr: unused)
  const char* r;      // residual bytes of the tile's first output row (nullptr: unused)
  int ne, elim;       // chunks per epilogue tensor; bytes valid from m / r (rows past the item read 0)
};

template <class T, int C, int PV>
struct TileRegs {
  static constexpr int VEC = 16 / (int)sizeof(T), CPR = C / VEC;
  uint4 v[PV];
  unsigned ok;  // bit i: chunk i is real data (else it is stored as zeros)
  // Branch-free: every chunk issues its load (an out-of-range chunk reads a valid dummy address and is
  // zeroed at store time) so the PV loads go out back to back. A per-chunk `if (valid) load` makes hipcc
  // branch around each load and wait vmcnt(0) per chunk (cdna_hip_programming.md, trap (c)).
  __device__ __forceinline__ void load(const TileSrc& s, int T_in) {
    ok = 0u;
#pragma unroll
    for (int i = 0; i < PV; ++i) {
      const int e = threadIdx.x + i * 256;
      const int row = e / CPR, q = e % CPR, gr = s.r0 + row;
      const bool in_x = e < s.nx;
      const bool vx = in_x && gr >= 0 && gr < T_in;
      const int e2 = e - s.nx;
      const bool in_m = s.m != nullptr && e2 < s.ne;
      const int e3 = s.m != nullptr ? e2 - s.ne : e2;
      const int ei = in_m ? e2 : e3;
      const char* eb = in_m ? s.m : s.r;
      const bool ve = !in_x && eb != nullptr && ei < s.ne && ei * 16 < s.elim;
      const char* px = s.x + (long long)gr * C * (int)sizeof(T) + q * 16;
      const char* pe = eb + (long long)ei * 16;
      const char* p = vx ? px : (ve ? pe : s.x);
      v[i] = *(const uint4*)p;
      ok |= (vx || ve) ? (1u << i) : 0u;
    }
  }
  __device__ __forceinline__ void store(const TileSrc& s, T* xl, int XS, char* ml, char* rl, bool relu) {
#pragma unroll
    for (int i = 0; i < PV; ++i) {
      const int e = threadIdx.x + i * 256;
      uint4 t = v[i];
      if (!(ok & (1u << i))) t = uint4{0u, 0u, 0u, 0u};
      if (e < s.nx) {
        const int row = e / CPR, q = e % CPR;
        if (relu) relu_bits<T>(t);
        *(uint4*)(xl + row * XS + q * VEC) = t;
      } else {
        int e2 = e - s.nx;
        char* b = s.m ? ml : nullptr;
        if (!b || e2 >= s.ne) {
          if (s.m) e2 -= s.ne;
          b = s.r ? rl : nullptr;
        }
        if (b && e2 < s.ne) *((uint4*)b + e2) = t;
      }
    }
  }
};


// MFMA gather conv, persistent and software-pipelined. Each workgroup (4 waves) owns a contiguous range
// of TM-row tiles of one or more items (a tile's halo rows were just read by its predecessor on the
// same CU), stages the weights once, and keeps TWO tiles in flight in registers (tiles i+1, i+2) while
// tile i runs its MFMAs and epilogue out of LDS — so neither the input rows nor the epilogue operands
// (residual, ReLU' mask) are ever waited for inside a tile (cdna_hip_programming.md T14, two deep).
// D[o][t] = sum_{k,c} Weff^T[o][(k,c)] * X[(k,c)][t]: A = weights (rows = output channels), B = a 16-byte
// channel run of one input row; each accumulator lane holds 4 consecutive output channels of one row.
// occupancy target: 4 waves/SIMD (<= 128 VGPRs) for the 4-chunk stager, 3 (<= 168) for 8, 2 for 12;
// O = 128 tiles (and fp32 O = 64 with 8 chunks) need more registers than that without spilling
template <class T, int O, int PV> constexpr int gather_waves() {
  if (O >= 128 || (sizeof(T) == 4 && O >= 64 && PV > 4)) return 2;
  return PV <= 4 ? 4 : (PV <= 5 ? (O <= 32 ? 4 : 3) : (PV <= 8 ? 3 : 2));
}

template <class T, int C, int O, int TM, int PV>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(gather_waves<T, O, PV>(), 8)))
void gather_mfma_kernel(GatherArgs a, int ntm, int ntiles, int tpw) {
  typedef Mfma<T> M;
  constexpr int NW = 4, RW = TM / NW, NT = RW / 16, MT = O / 16;
  constexpr int XS = C + lds_pad<T>();
  constexpr int WS = C + lds_pad<T>();
  static_assert(RW % 16 == 0 && O % 16 == 0 && C % M::KS == 0, "tile shape");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* wl = (T*)smem;
  T* xl = wl + (size_t)a.K * O * WS;
  const int rows_in = (TM - 1) * a.S + (a.K - 1) * a.D + 1;
  // epilogue tiles, unpadded and chunk-linear: [TM][O], or in PAIR mode [2TM][O/2] (full-resolution rows)
  T* ml = xl + (size_t)rows_in * XS;
  T* rl = ml + (size_t)TM * O;

  const int tbeg = blockIdx.x * tpw, tend = min(ntiles, tbeg + tpw);
  if (tbeg >= tend) return;
  const bool pair = a.wmode == W_PAIR;
  const bool do_mask = a.flags & VQA_POST_MASK, do_res = a.flags & VQA_ADD_RESIDUAL;
  const bool relu = a.flags & VQA_PRE_RELU;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int ko = M::koff(lane);
  constexpr int ESZ = (int)sizeof(T);
  const int erow = pair ? O / 2 : O;  // elements per output row (full resolution)

  auto source = [&](int tile) {
    const int n = tile / ntm, t0 = (tile - n * ntm) * TM;
    TileSrc src;
    src.x = (const char*)a.x + (long long)n * a.T_in * C * ESZ;
    src.r0 = t0 * a.S - a.P;
    src.nx = rows_in * (C * ESZ / 16);
    const int r0e = pair ? 2 * t0 : t0;                 // first output row of the tile
    const int rvalid = pair ? a.T_full : a.T_out;        // output rows of this item
    const long long eoff = ((long long)n * rvalid + r0e) * erow * ESZ;
    src.m = do_mask ? (const char*)a.mask + eoff : nullptr;
    src.r = do_res ? (const char*)a.resid + eoff : nullptr;
    src.ne = TM * O * ESZ / 16;
    src.elim = (rvalid - r0e) * erow * ESZ;
    return src;
  };

  // the bias per output channel (PAIR: both halves), staged once: the epilogue reads it from LDS (a global load
  // per output block in the epilogue was waited for in turn: 8 serial round trips per tile at O = 128)
  __shared__ __attribute__((aligned(16))) float bias_l[O];
  for (int i = threadIdx.x; i < O; i += 256) bias_l[i] = a.bias ? a.bias[bias_index(a, i)] : 0.f;
  stage_weights<T, C, O>(a, wl, WS);
  TileSrc S0, S1;
  TileRegs<T, C, PV> A, B;
  S0 = source(tbeg);
  A.load(S0, a.T_in);
  if (tbeg + 1 < tend) {
    S1 = source(tbeg + 1);
    B.load(S1, a.T_in);
  }
  A.store(S0, xl, XS, (char*)ml, (char*)rl, relu);
  __syncthreads();

  // bf16 tiles without epilogue operands: the output rows staged in the (then unused) epilogue-operand region and
  // stored as contiguous 16-byte chunks (the 8-byte per-lane stores wrote a quarter of a cache line each)
  constexpr int OP = O + 8;
  const int rvalid_ = pair ? a.T_full : a.T_out;
  const bool se = sizeof(T) == 2 && !do_mask && !do_res && (long long)rvalid_ * erow * ESZ < (1ll << 31);
  T* stg = ml + (size_t)wave * RW * OP;
  static_assert(TM * (O + 8) <= 2 * TM * O, "staged tile fits the two epilogue-operand tiles");

  // one tile: MFMAs out of LDS, epilogue operands out of LDS, stores to global
  auto run_tile = [&](int tile) {
    const int n = tile / ntm, t0 = (tile - n * ntm) * TM;
    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {  // K <= 4 (host-checked): unrolled, uniform exit
      if (k >= a.K) break;
      const T* wk = wl + (size_t)k * O * WS + (lane & 15) * WS + ko;
      const T* xk = xl + (size_t)(k * a.D) * XS + ko;
#pragma unroll
      for (int cc = 0; cc < C; cc += M::KS) {
        typename M::frag af[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) af[mt] = M::load(wk + mt * 16 * WS + cc);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const int tl = wave * RW + nt * 16 + (lane & 15);
          const typename M::frag bf = M::load(xk + (size_t)(tl * a.S) * XS + cc);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = M::mma(af[mt], bf, acc[mt][nt]);
        }
      }
    }
    if (se) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const int o = mt * 16 + 4 * (lane >> 4);
          f32x4 v = acc[mt][nt];
          if (a.bias) {
            const f32x4 bp = *(const f32x4*)(bias_l + o);
            v = f32x4{v[0] + bp[0], v[1] + bp[1], v[2] + bp[2], v[3] + bp[3]};
          }
          const bf16x4 ob = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
          *(bf16x4*)(stg + (nt * 16 + (lane & 15)) * OP + o) = ob;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      // the wave's RW output rows are contiguous (PAIR: row t holds full-resolution rows 2t, 2t+1); rows past the
      // item are dropped by the range check (a 16-byte chunk never straddles a PAIR half)
      const unsigned ib = (unsigned)((long long)rvalid_ * erow * ESZ);
      const __amdgpu_buffer_rsrc_t ry = item_rsrc(a.y, (long long)n * ib, ib);
      constexpr int CPRO = O * 2 / 16, NCH = RW * CPRO / 64;
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int e = lane + 64 * i, r = e / CPRO, q = e - r * CPRO;
        const u32x4 c = *(const u32x4*)(stg + r * OP + q * 8);
        __builtin_amdgcn_raw_buffer_store_b128(c, ry, ((t0 + wave * RW + r) * O + q * 8) * 2, 0, 0);
      }
      return;
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int tl = wave * RW + nt * 16 + (lane & 15);
      const int t = t0 + tl;
      if (t >= a.T_out) continue;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int o = mt * 16 + 4 * (lane >> 4);
        const long long oi = out_index(a, n, t, o);
        if (oi < 0) continue;
        // this element inside the staged (unpadded) epilogue tile
        int eidx;
        if (pair) {
          const int Ob = O / 2, p = o >= Ob ? 1 : 0;
          eidx = (2 * tl + p) * Ob + (o - p * Ob);
        } else {
          eidx = tl * O + o;
        }
        f32x4 v = acc[mt][nt];
        if (a.bias) {
          const f32x4 bp = *(const f32x4*)(bias_l + o);
          v = f32x4{v[0] + bp[0], v[1] + bp[1], v[2] + bp[2], v[3] + bp[3]};
        }
        if (do_mask) {
          const f32x4 m = ld4(ml + eidx);
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = m[i] > 0.f ? v[i] : 0.f;
        }
        if (do_res) {
          const f32x4 r = ld4(rl + eidx);
          v = f32x4{r[0] + v[0], r[1] + v[1], r[2] + v[2], r[3] + v[3]};
        }
        st4((T*)a.y + oi, v);
      }
    }
  };

  // steady state, unrolled by two so each register set has a static name (rule 20)
  for (int tile = tbeg; tile < tend; tile += 2) {
    // LDS: tile; B: tile+1 (in flight); A: free
    if (tile + 2 < tend) {
      S0 = source(tile + 2);
      A.load(S0, a.T_in);
    }
    run_tile(tile);
    __syncthreads();
    if (tile + 1 >= tend) break;
    B.store(S1, xl, XS, (char*)ml, (char*)rl, relu);
    __syncthreads();
    // LDS: tile+1; A: tile+2 (in flight); B: free
    if (tile + 3 < tend) {
      S1 = source(tile + 3);
      B.load(S1, a.T_in);
    }
    run_tile(tile + 1);
    __syncthreads();
    if (tile + 2 >= tend) break;
    A.store(S0, xl, XS, (char*)ml, (char*)rl, relu);
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------
// The 32-channel residual convs (C = O = 32, direct or stride-1 data-gradient weights, any K <= 4,
// stride 1 or 2) — 80 % of the model's conv traffic — get a leaner kernel than gather_mfma_kernel:
//  * every global access is a raw buffer access through a per-item descriptor, so the hardware range
//    check supplies the SAME zero padding and drops stores past the item end (no per-element guards);
//  * all per-thread chunk offsets are computed once per launch: staging costs one add per 16-byte chunk
//    and the epilogue tensors (ReLU' mask / conv input, residual) are plain contiguous spans;
//  * the ReLU is one packed integer max per dword (a bf16 / fp32 is negative iff its int16 / int32 is);
//  * the tile is held in registers two tiles ahead (T14) exactly as in gather_mfma_kernel.
// FW additionally accumulates the weight gradient of a stride-1 data-gradient from the staged tiles
// (vqa_conv1d_bwd_data_weight): epilogue tensor 0 is then the conv input u.
template <class T> __device__ __forceinline__ u32x4 relu_chunk(u32x4 v);
__device__ __forceinline__ unsigned relu_pk_bf16(unsigned w) {
  const s16x2 z = {0, 0};
  return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(s16x2, w), z));
}
template <> __device__ __forceinline__ u32x4 relu_chunk<bf16>(u32x4 v) {
  return u32x4{relu_pk_bf16(v.x), relu_pk_bf16(v.y), relu_pk_bf16(v.z), relu_pk_bf16(v.w)};
}
__device__ __forceinline__ unsigned relu_f32_bits(unsigned w) { return (unsigned)max((int)w, 0); }
template <> __device__ __forceinline__ u32x4 relu_chunk<float>(u32x4 v) {
  return u32x4{relu_f32_bits(v.x), relu_f32_bits(v.y), relu_f32_bits(v.z), relu_f32_bits(v.w)};
}

template <class T> __device__ __forceinline__ void store_out4(__amdgpu_buffer_rsrc_t r, int voff, f32x4 v);
template <> __device__ __forceinline__ void store_out4<bf16>(__amdgpu_buffer_rsrc_t r, int voff, f32x4 v) {
  bf16x4 o = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, o), r, voff, 0, 0);
}
template <> __device__ __forceinline__ void store_out4<float>(__amdgpu_buffer_rsrc_t r, int voff, f32x4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, voff, 0, 0);
}

template <class T, int O, int PVX, int NEP, bool FW> constexpr int conv32_waves() {
  if (FW) return sizeof(T) == 2 ? 3 : 2;
  const int regs = PVX + NEP * (int)sizeof(T) * (O / 32) + (O / 32 - 1) * 4;
  return regs <= 7 ? 4 : (regs <= 11 ? 3 : 2);
}

// bf16 output tiles (no fused weight gradient) are staged through LDS over the x rows before they are stored: each
// lane then writes whole 16-byte chunks of contiguous output rows (1 KB per wave store) instead of 8-byte pieces of
// 16 rows (a quarter of a cache line each); the x region is sized for the staged tile (row pitch O + 8)
template <class T, bool FW> constexpr bool conv32_staged() { return !FW && sizeof(T) == 2; }
template <class T, int O, int PVX, bool FW> constexpr int conv32_xelems() {
  constexpr int XS = 32 + 16 / (int)sizeof(T), XROWS = 256 / (32 / (16 / (int)sizeof(T))) * PVX;
  return conv32_staged<T, FW>() && 128 * (O + 8) > XROWS * XS ? 128 * (O + 8) : XROWS * XS;
}

// O = 64: a 32 -> 64 conv, or the PAIR layout (conv-transpose forward, stride-2 data-gradient) whose
// output row j holds the two full-resolution rows 2j, 2j+1 (32 channels each) — the bytes of (B, 2T, 32).
template <class T, int O, int PVX, int NEP, bool FW>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(conv32_waves<T, O, PVX, NEP, FW>(), 8)))
void conv32_kernel(GatherArgs a, int ntm, int ntiles, int tpw) {
  typedef Mfma<T> M;
  static_assert(O == 32 || (O == 64 && !FW), "conv32: O = 32 or 64 (64 without FW)");
  constexpr int C = 32, TM = 128, NW = 4, RW = TM / NW, NT = RW / 16, MT = O / 16;
  constexpr int ESZ = (int)sizeof(T), VEC = 16 / ESZ, CPR = C / VEC, ROWB = C * ESZ;
  constexpr int XS = C + lds_pad<T>(), WS = XS;
  constexpr int RSTEP = 256 / CPR;  // x rows between a thread's consecutive chunks
  constexpr int XROWS = RSTEP * PVX;
  constexpr int ECH = TM * O * ESZ / 16 / 256;  // chunks per thread per epilogue tensor
  constexpr int EBYTES = TM * O * ESZ;
  static_assert(NEP >= (FW ? 1 : 0) && NEP <= 2, "epilogue tensors");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* wl = (T*)smem;
  T* xl = wl + (size_t)a.K * O * WS;
  char* el = (char*)(xl + (size_t)conv32_xelems<T, O, PVX, FW>());
  constexpr bool SE = conv32_staged<T, FW>();
  constexpr int OP = O + 8;  // staged row pitch (elements)

  const int tbeg = blockIdx.x * tpw, tend = min(ntiles, tbeg + tpw);
  if (tbeg >= tend) return;
  const bool do_mask = a.flags & VQA_POST_MASK, do_res = a.flags & VQA_ADD_RESIDUAL;
  const bool relu = a.flags & VQA_PRE_RELU;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int ko = M::koff(lane);
  const int rows_in = (TM - 1) * a.S + (a.K - 1) * a.D + 1;
  // epilogue tensor slots: [mask or conv input (FW)] then [residual]
  const bool has_m = do_mask || FW;
  const void* ep0 = has_m ? a.mask : a.resid;
  const void* ep1 = a.resid;
  const T* ml = (const T*)el;                                   // valid when has_m
  const T* rl = (const T*)(el + (has_m ? EBYTES : 0));          // valid when do_res
  const unsigned xbytes = (unsigned)a.T_in * ROWB;
  // PAIR: the item's valid bytes end at full-resolution row T_full (the range check drops the rest)
  const bool pair = a.wmode == W_PAIR;
  const unsigned obytes = pair ? (unsigned)a.T_full * (O / 2) * ESZ : (unsigned)a.T_out * O * ESZ;

  // per-thread chunk geometry, fixed for the launch
  const int q = threadIdx.x % CPR, row0 = threadIdx.x / CPR;
  int gx[PVX];
#pragma unroll
  for (int i = 0; i < PVX; ++i) gx[i] = (row0 + i * RSTEP < rows_in) ? (row0 + i * RSTEP) * ROWB + q * 16 : kOOB;
  const int lx = (row0 * XS) * ESZ + q * 16;  // + i * RSTEP * XS * ESZ
  const int ge = threadIdx.x * 16;            // + j * 4096 (epilogue chunks)

  u32x4 ra[PVX + NEP * ECH], rb[PVX + NEP * ECH];
  auto load = [&](u32x4* r, int tile) {
    const int n = tile / ntm, t0 = (tile - n * ntm) * TM;
    const __amdgpu_buffer_rsrc_t rx = item_rsrc(a.x, (long long)n * xbytes, xbytes);
    const int xb = (t0 * a.S - a.P) * ROWB;
#pragma unroll
    for (int i = 0; i < PVX; ++i) r[i] = __builtin_amdgcn_raw_buffer_load_b128(rx, gx[i] + xb, 0, 0);
    if constexpr (NEP > 0) {
      const int eb = t0 * O * ESZ;
      const __amdgpu_buffer_rsrc_t r0 = item_rsrc(ep0, (long long)n * obytes, obytes);
#pragma unroll
      for (int j = 0; j < ECH; ++j) r[PVX + j] = __builtin_amdgcn_raw_buffer_load_b128(r0, ge + j * 4096 + eb, 0, 0);
      if constexpr (NEP > 1) {
        const __amdgpu_buffer_rsrc_t r1 = item_rsrc(ep1, (long long)n * obytes, obytes);
#pragma unroll
        for (int j = 0; j < ECH; ++j)
          r[PVX + ECH + j] = __builtin_amdgcn_raw_buffer_load_b128(r1, ge + j * 4096 + eb, 0, 0);
      }
    }
  };
  auto store = [&](const u32x4* r) {
#pragma unroll
    for (int i = 0; i < PVX; ++i)
      *(u32x4*)((char*)xl + lx + i * RSTEP * XS * ESZ) = relu ? relu_chunk<T>(r[i]) : r[i];
#pragma unroll
    for (int j = 0; j < NEP * ECH; ++j) *(u32x4*)(el + ge + j * 4096) = r[PVX + j];
  };

  // fused weight gradient accumulators (C = O = 32: wave w owns ci-tile w>>1, co-tile w&1 of every tap)
  f32x4 wacc[4], wdb = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; ++i) wacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  // bias of this lane's 4 output channels per 16-channel block
  f32x4 bias[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int o = mt * 16 + 4 * (lane >> 4), bo = pair ? (o & (O / 2 - 1)) : o;  // PAIR: halves share the bias
    bias[mt] = a.bias ? f32x4{a.bias[bo], a.bias[bo + 1], a.bias[bo + 2], a.bias[bo + 3]} : f32x4{0.f, 0.f, 0.f, 0.f};
  }

  stage_weights<T, C, O>(a, wl, WS);
  load(ra, tbeg);
  if (tbeg + 1 < tend) load(rb, tbeg + 1);
  store(ra);
  __syncthreads();

  auto run_tile = [&](int tile) {
    const int n = tile / ntm, t0 = (tile - n * ntm) * TM;
    // the accumulators start at the bias (the fused residual block's convs do the same: bit-identical outputs)
    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[i][j] = bias[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {  // K <= 4 (host-checked): unrolled, uniform exit
      if (k >= a.K) break;
      const T* wk = wl + (size_t)k * O * WS + (lane & 15) * WS + ko;
      const T* xk = xl + (size_t)(k * a.D) * XS + ko;
#pragma unroll
      for (int cc = 0; cc < C; cc += M::KS) {
        typename M::frag af[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) af[mt] = M::load(wk + mt * 16 * WS + cc);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const int tl = wave * RW + nt * 16 + (lane & 15);
          const typename M::frag bf = M::load(xk + (size_t)(tl * a.S) * XS + cc);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = M::mma(af[mt], bf, acc[mt][nt]);
        }
      }
    }
    const __amdgpu_buffer_rsrc_t ry = item_rsrc(a.y, (long long)n * obytes, obytes);
    const int yb = t0 * O * ESZ;
    T* stg = xl + (size_t)wave * RW * OP;  // SE: this wave's staged rows
    if constexpr (SE) __syncthreads();     // every wave's MFMA reads of the x rows are done
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int tl = wave * RW + nt * 16 + (lane & 15);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int o = mt * 16 + 4 * (lane >> 4);
        const int eidx = tl * O + o;
        f32x4 v = acc[mt][nt];
        if (do_mask) {
          const f32x4 m = ld4(ml + eidx);
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = m[i] > 0.f ? v[i] : 0.f;
        }
        if (do_res) v = ld4(rl + eidx) + v;
        if constexpr (SE) {
          const bf16x4 ob = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
          *(bf16x4*)(stg + (nt * 16 + (lane & 15)) * OP + o) = ob;
        } else {
          store_out4<T>(ry, eidx * ESZ + yb, v);
        }
      }
    }
    if constexpr (SE) {
      // the wave's RW rows are contiguous in the output: 16-byte chunks, rows past the item dropped by the range
      // check (a chunk never straddles a PAIR half: 32 channels = 4 chunks)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      constexpr int CPRO = O * 2 / 16, NCH = RW * CPRO / 64;
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int e = lane + 64 * i, r = e / CPRO, q = e - r * CPRO;
        const u32x4 c = *(const u32x4*)(stg + r * OP + q * 8);
        __builtin_amdgcn_raw_buffer_store_b128(c, ry, ((wave * RW + r) * O + q * 8) * 2 + yb, 0, 0);
      }
    }
    if constexpr (FW) {
      const int it = wave >> 1, jt = wave & 1;
      const T* up = ml + it * 16;
      const T* gp = xl + jt * 16;
#pragma unroll 1
      for (int kk = 0; kk < TM; kk += M::KS) {
        typename M::frag af = M::rows(up + (size_t)kk * O, O);
        if (a.wrelu) af = relu_frag(af);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (k < a.K) {
            const typename M::frag bf = M::rows(gp + (size_t)(kk + (a.K - 1 - k) * a.D) * XS, XS);
            wacc[k] = M::mma(af, bf, wacc[k]);
          }
        }
        if (it == 0) {
          const typename M::frag bo = M::rows(gp + (size_t)(kk + a.P) * XS, XS);
          wdb = M::mma(M::ones(), bo, wdb);
        }
      }
    }
  };

  for (int tile = tbeg; tile < tend; tile += 2) {
    // LDS: tile; rb: tile+1 (in flight); ra: free
    if (tile + 2 < tend) load(ra, tile + 2);
    run_tile(tile);
    __syncthreads();
    if (tile + 1 >= tend) break;
    store(rb);
    __syncthreads();
    if (tile + 3 < tend) load(rb, tile + 3);
    run_tile(tile + 1);
    __syncthreads();
    if (tile + 2 >= tend) break;
    store(ra);
    __syncthreads();
  }
  if constexpr (FW) {
    float* out = a.wpart + (size_t)blockIdx.x * (size_t)(a.K * O * C + C);
    const int it = wave >> 1, jt = wave & 1;
    const int co = jt * 16 + (lane & 15);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < a.K) {
#pragma unroll
        for (int r = 0; r < 4; ++r) out[((size_t)k * O + it * 16 + 4 * (lane >> 4) + r) * C + co] = wacc[k][r];
      }
    }
    if (it == 0 && lane < 16) out[a.K * O * C + co] = wdb[0];
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// rows per workgroup tile: all O channels x TM rows; TM keeps VGPRs <= ~128 (3 waves/SIMD)
static int gather_tm(int O, int S) {
  (void)S;
  return O == 32 ? 128 : 64;
}

// persistent grid = the resident workgroups (VGPR- and LDS-limited), so no workgroup waits for a second
// round; tiles are split into contiguous ranges (a tile's halo rows were just read by its predecessor)
static int persistent_grid(const void* fn, size_t lds, int ntiles, int* tpw) {
  int nwg = cu_count() * std::min(resident_per_cu(fn, 256, lds), kMaxGatherPerCU);
  if (nwg > ntiles) nwg = ntiles;
  *tpw = (ntiles + nwg - 1) / nwg;
  return (ntiles + *tpw - 1) / *tpw;
}

template <class T, int C, int O, int TM, int PV>
static int launch_gather_mfma_pv(const GatherArgs& a, size_t lds, hipStream_t s) {
  const void* fn = (const void*)gather_mfma_kernel<T, C, O, TM, PV>;
  const int rc = raise_dyn_lds(fn, lds, "gather_mfma_kernel");
  if (rc != VQA_OK) return rc;
  const int ntm = (a.T_out + TM - 1) / TM;
  const int ntiles = ntm * a.B;
  int tpw = 0;
  const int nwg = persistent_grid(fn, lds, ntiles, &tpw);
  hipLaunchKernelGGL((gather_mfma_kernel<T, C, O, TM, PV>), dim3(nwg), dim3(256), lds, s, a, ntm, ntiles, tpw);
  VQA_LAUNCHED("gather_mfma_kernel");
  return VQA_OK;
}

// epilogue tiles staged per tile: ReLU' mask / conv input (fused wgrad), residual
int gather_nep(const GatherArgs& a, bool fw) {
  return (((a.flags & VQA_POST_MASK) || fw) ? 1 : 0) + ((a.flags & VQA_ADD_RESIDUAL) ? 1 : 0);
}

// channel counts and taps the MFMA kernel is built for (its tap loop is unrolled for K <= 4)
static bool mfma_channels(const GatherArgs& a) {
  return a.K <= 4 && (a.C == 32 || a.C == 64) && (a.O == 32 || a.O == 64 || a.O == 128);
}

static MfmaPlan mfma_plan(const GatherArgs& a, int dtype) {
  MfmaPlan p{};
  if ((uintptr_t)a.w & 15) return p;  // stage_weights reads the kernel in 16-byte vectors
  if (a.flags & (VQA_X_F32 | VQA_Y_F32)) return p;
  if (!mfma_channels(a)) return p;
  p.tm = gather_tm(a.O, a.S);
  p.nep = gather_nep(a, false);
  const int rows_in = (p.tm - 1) * a.S + (a.K - 1) * a.D + 1;
  const int esz = dtype == VQA_BF16 ? 2 : 4;
  // 16-byte chunks per tile held in registers per thread; a tile only a few chunks over a multiple of
  // 256 must not pay for the next size up
  const long long chunks = (long long)rows_in * a.C * esz / 16 + (long long)p.nep * p.tm * a.O * esz / 16;
  if (chunks > 12 * 256) return p;
  if ((size_t)rows_in * (a.C + 8) * 4 + (size_t)a.K * a.O * (a.C + 8) * 4 > 150 * 1024) return p;
  // the kernel's own LDS: weights, input rows (row pitch C + 16 bytes) and the two epilogue-operand tiles. A tile
  // that does not fit (fp32 C = 64 -> O = 128: the width-64 transposed conv and stride-2 data gradient) is not an
  // MFMA conv
  const int pitch = a.C + 16 / esz;
  p.lds = ((size_t)a.K * a.O * pitch + (size_t)rows_in * pitch) * esz + 2 * (size_t)p.tm * a.O * esz;
  if (p.lds > 160 * 1024) return p;
  const int pv = (int)((chunks + 255) / 256);
  p.pv = pv <= 3 ? 3 : (pv <= 4 ? 4 : (pv <= 5 ? 5 : (pv <= 8 ? 8 : 12)));
  p.ok = true;
  return p;
}

template <class T, int C, int O, int TM>
static int launch_gather_mfma_t(const GatherArgs& a, const MfmaPlan& p, hipStream_t s) {
  static_assert(C + lds_pad<T>() == C + 16 / (int)sizeof(T), "mfma_plan's row pitch");
  VQA_REQUIRE(p.ok && p.tm == TM, VQA_E_UNSUPPORTED, "gather conv: no MFMA plan for this tile");
  switch (p.pv) {
    case 3: return launch_gather_mfma_pv<T, C, O, TM, 3>(a, p.lds, s);
    case 4: return launch_gather_mfma_pv<T, C, O, TM, 4>(a, p.lds, s);
    case 5: return launch_gather_mfma_pv<T, C, O, TM, 5>(a, p.lds, s);
    case 8: return launch_gather_mfma_pv<T, C, O, TM, 8>(a, p.lds, s);
    default: return launch_gather_mfma_pv<T, C, O, TM, 12>(a, p.lds, s);
  }
}

template <class T, int C, int O>
static int launch_gather_mfma_o(const GatherArgs& a, const MfmaPlan& p, hipStream_t s) {
  if constexpr (O == 32) return launch_gather_mfma_t<T, C, O, 128>(a, p, s);
  else return launch_gather_mfma_t<T, C, O, 64>(a, p, s);
}

template <class T>
static int launch_gather_mfma(const GatherArgs& a, const MfmaPlan& p, hipStream_t s) {
  if (a.C == 32) {
    if (a.O == 32) return launch_gather_mfma_o<T, 32, 32>(a, p, s);
    if (a.O == 64) return launch_gather_mfma_o<T, 32, 64>(a, p, s);
    if (a.O == 128) return launch_gather_mfma_o<T, 32, 128>(a, p, s);
  } else if (a.C == 64) {
    if (a.O == 32) return launch_gather_mfma_o<T, 64, 32>(a, p, s);
    if (a.O == 64) return launch_gather_mfma_o<T, 64, 64>(a, p, s);
    if (a.O == 128) return launch_gather_mfma_o<T, 64, 128>(a, p, s);
  }
  vqa::set_error("gather conv: no MFMA tile for C=%d O=%d", a.C, a.O);
  return VQA_E_UNSUPPORTED;
}

// ---- the 32-channel kernel
template <class T, int O, int PVX, int NEP, bool FW>
static int launch_conv32_k(const GatherArgs& a, hipStream_t s, int* nwg_out) {
  constexpr int ESZ = (int)sizeof(T), XS = 32 + lds_pad<T>();
  const size_t lds = ((size_t)a.K * O * XS + (size_t)conv32_xelems<T, O, PVX, FW>()) * ESZ + (size_t)NEP * 128 * O * ESZ;
  const void* fn = (const void*)conv32_kernel<T, O, PVX, NEP, FW>;
  const int rc = raise_dyn_lds(fn, lds, "conv32_kernel");
  if (rc != VQA_OK) return rc;
  const int ntm = (a.T_out + 127) / 128;
  const int ntiles = ntm * a.B;
  int tpw = 0;
  const int nwg = persistent_grid(fn, lds, ntiles, &tpw);
  if (nwg_out) *nwg_out = nwg;
  hipLaunchKernelGGL((conv32_kernel<T, O, PVX, NEP, FW>), dim3(nwg), dim3(256), lds, s, a, ntm, ntiles, tpw);
  VQA_LAUNCHED("conv32_kernel");
  return VQA_OK;
}

template <class T, int PVX, bool FW>
static int launch_conv32_n(const GatherArgs& a, int nep, hipStream_t s, int* nwg_out) {
  if constexpr (!FW) {
    if (a.O == 64) {
      if (nep == 0) return launch_conv32_k<T, 64, PVX, 0, false>(a, s, nwg_out);
      if (nep == 1) return launch_conv32_k<T, 64, PVX, 1, false>(a, s, nwg_out);
      return launch_conv32_k<T, 64, PVX, 2, false>(a, s, nwg_out);
    }
    if (nep == 0) return launch_conv32_k<T, 32, PVX, 0, FW>(a, s, nwg_out);
  }
  if (nep == 1) return launch_conv32_k<T, 32, PVX, 1, FW>(a, s, nwg_out);
  return launch_conv32_k<T, 32, PVX, 2, FW>(a, s, nwg_out);
}

// x chunks per thread the 32-channel kernel stages for this launch (0: not applicable)
int conv32_pvx(const GatherArgs& a, int dtype, bool fw) {
  if ((uintptr_t)a.w & 15) return 0;  // stage_weights reads the kernel in 16-byte vectors
  const bool o64 = a.O == 64 && !fw && (a.wmode != W_PAIR || a.T_full <= 2 * a.T_out);
  if (a.C != 32 || !((a.O == 32 && a.wmode != W_PAIR) || o64) || a.K > 4 || a.S > 2) return 0;
  if (a.flags & (VQA_X_F32 | VQA_Y_F32)) return 0;
  if (fw && (a.S != 1 || a.K > 3 || a.wmode != W_FLIP_T)) return 0;
  const int esz = dtype == VQA_BF16 ? 2 : 4;
  if ((long long)a.T_in * 32 * esz >= (1ll << 29) || (long long)a.T_out * a.O * esz >= (1ll << 29)) return 0;
  const int rows_in = 127 * a.S + (a.K - 1) * a.D + 1;
  const int chunks = rows_in * 32 * esz / 16;
  const int pv = (chunks + 255) / 256;
  const int opts_bf16[] = {3, 5}, opts_f32[] = {5, 6, 9};
  const int* opts = esz == 2 ? opts_bf16 : opts_f32;
  const int nopt = esz == 2 ? 2 : 3;
  for (int i = 0; i < nopt; ++i) {
    if (pv <= opts[i]) {
      const int xs = 32 + 16 / esz, xrows = 256 / (32 * esz / 16) * opts[i];
      const size_t lds = ((size_t)a.K * a.O * xs + (size_t)xrows * xs) * esz + 2 * 128 * (size_t)a.O * esz;
      return lds <= 150 * 1024 ? opts[i] : 0;
    }
  }
  return 0;
}

template <class T, bool FW>
static int launch_conv32(const GatherArgs& a, int pvx, hipStream_t s, int* nwg_out) {
  const int nep = gather_nep(a, FW);
  if constexpr (sizeof(T) == 2) {
    if (pvx == 3) return launch_conv32_n<T, 3, FW>(a, nep, s, nwg_out);
    return launch_conv32_n<T, 5, FW>(a, nep, s, nwg_out);
  } else {
    if (pvx == 5) return launch_conv32_n<T, 5, FW>(a, nep, s, nwg_out);
    if (pvx == 6) return launch_conv32_n<T, 6, FW>(a, nep, s, nwg_out);
    return launch_conv32_n<T, 9, FW>(a, nep, s, nwg_out);
  }
}

template <class TX, class TY>
static int launch_gather_direct(const GatherArgs& a, hipStream_t s) {
  const long long total = (long long)a.B * a.T_out * a.O;
  long long blocks = (total + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL((gather_direct_kernel<TX, TY>), dim3((unsigned)blocks), dim3(256), 0, s, a);
  VQA_LAUNCHED("gather_direct_kernel");
  return VQA_OK;
}

template <class TX, class TY, int C>
static int launch_gather_thinO_c(const GatherArgs& a, hipStream_t s) {
  const int ntb = (a.T_out + 255) / 256;
  const int rows_in = 255 * a.S + (a.K - 1) * a.D + 1;
  const size_t lds = ((size_t)a.K * C * a.O * 4 + 15) / 16 * 16 + (size_t)rows_in * (C + 16 / sizeof(TX)) * sizeof(TX);
  const int rc = raise_dyn_lds((const void*)gather_thinO_kernel<TX, TY, C>, lds, "gather_thinO_kernel");
  if (rc != VQA_OK) return rc;
  hipLaunchKernelGGL((gather_thinO_kernel<TX, TY, C>), dim3(ntb * a.B), dim3(256), lds, s, a, ntb);
  VQA_LAUNCHED("gather_thinO_kernel");
  return VQA_OK;
}

template <class TX, class TY>
static int launch_gather_thinO(const GatherArgs& a, hipStream_t s) {
  return a.C == 32 ? launch_gather_thinO_c<TX, TY, 32>(a, s) : launch_gather_thinO_c<TX, TY, 64>(a, s);
}

// the thin kernel indexes its (row, channel group) items with 32-bit integers
bool gather_thin_fits(const GatherArgs& a) { return (long long)a.B * a.T_out * a.O < (1ll << 31); }

template <class TX, class TY>
static int launch_gather_thin(const GatherArgs& a, hipStream_t s) {
  VQA_REQUIRE(gather_thin_fits(a), VQA_E_UNSUPPORTED, "thin conv: tensor too large");
  const int OV = (a.O % 8 == 0) ? 8 : 1;
  const long long total = (long long)a.B * a.T_out * (a.O / OV);
  long long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  if (blocks < 1) blocks = 1;
  const size_t lds = (size_t)a.K * a.C * a.O * sizeof(float);
  if (OV == 8)
    hipLaunchKernelGGL((gather_thin_kernel<TX, TY, 8>), dim3((unsigned)blocks), dim3(256), lds, s, a);
  else
    hipLaunchKernelGGL((gather_thin_kernel<TX, TY, 1>), dim3((unsigned)blocks), dim3(256), lds, s, a);
  VQA_LAUNCHED("gather_thin_kernel");
  return VQA_OK;
}

// ------------------------------------------------------------------------------------------------
// One-input-channel conv (the encoder's first conv on the waveform, encdec.py:33 with C = 1): a workgroup
// owns CI1_RB output rows of one item; their input span is staged once in LDS (fp32), each lane holds the
// K x 8 weights of its 8 output channels in registers and writes its rows' 8 channels as one 16-byte
// (bf16) store — consecutive lanes write consecutive bytes. Per-row tap order k = 0..K-1 (as the gather
// kernels).
constexpr int CI1_RB = 512, CI1_KMAX = 8;
// input values staged per thread by the unrolled path (span <= 256 CI1_SPT: stride 2, K <= 4 at CI1_RB = 512); the
// loads are issued together from clamped addresses, zeros selected (the loop form waited on every load in turn)
constexpr int CI1_SPT = 5;

// KT: the tap count as a compile-time constant (4: the model's first conv; fewer registers, all tap reads issued
// together) or 0 (any K <= CI1_KMAX from the arguments). Same sums in the same order either way.
template <class TX, class TY, int O, int KT>
__global__ __launch_bounds__(256) void gather_ci1_kernel(GatherArgs a) {
  constexpr int L = O / 8, RPP = 256 / L;  // lanes per row, rows per pass
  constexpr int KK = KT > 0 ? KT : CI1_KMAX;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* xl = (float*)smem;
  const int n = blockIdx.y, t0 = blockIdx.x * CI1_RB;
  const int span = (CI1_RB - 1) * a.S + (a.K - 1) * a.D + 1, i0 = t0 * a.S - a.P;
  const TX* X = (const TX*)a.x + (size_t)n * a.T_in;
  const bool relu = a.flags & VQA_PRE_RELU;
  if (span <= 256 * CI1_SPT) {
    float v[CI1_SPT];
#pragma unroll
    for (int i = 0; i < CI1_SPT; ++i) {
      const int e = threadIdx.x + 256 * i, ti = i0 + e;
      const bool ok = e < span && ti >= 0 && ti < a.T_in;
      const float x = ld(X + min(max(ti, 0), a.T_in - 1));
      v[i] = ok ? x : 0.f;
    }
#pragma unroll
    for (int i = 0; i < CI1_SPT; ++i) {
      const int e = threadIdx.x + 256 * i;
      if (e < span) xl[e] = relu ? fmaxf(v[i], 0.f) : v[i];
    }
  } else {
    for (int e = threadIdx.x; e < span; e += 256) {
      const int ti = i0 + e;
      float v = (ti >= 0 && ti < a.T_in) ? ld(X + ti) : 0.f;
      xl[e] = relu ? fmaxf(v, 0.f) : v;
    }
  }
  const int o8 = (threadIdx.x % L) * 8, rl = threadIdx.x / L;
  float w[KK][8], b[8];
#pragma unroll
  for (int k = 0; k < KK; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) w[k][j] = (KT > 0 || k < a.K) ? a.w[k * O + o8 + j] : 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) b[j] = a.bias ? a.bias[o8 + j] : 0.f;
  __syncthreads();
  TY* Y = (TY*)a.y + (size_t)n * a.T_out * O;
  for (int r = rl; r < CI1_RB && t0 + r < a.T_out; r += RPP) {
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
    for (int k = 0; k < KK; ++k) {
      if (KT == 0 && k >= a.K) break;
      const float xv = xl[r * a.S + k * a.D];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += xv * w[k][j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = acc[j] + b[j];
    st8(Y + (size_t)(t0 + r) * O + o8, acc);
  }
}

template <class TX, class TY, int KT>
static void launch_gather_ci1_k(const GatherArgs& a, const dim3& grid, size_t lds, hipStream_t s) {
  if (a.O == 32) hipLaunchKernelGGL((gather_ci1_kernel<TX, TY, 32, KT>), grid, dim3(256), lds, s, a);
  else hipLaunchKernelGGL((gather_ci1_kernel<TX, TY, 64, KT>), grid, dim3(256), lds, s, a);
}

template <class TX, class TY>
static int launch_gather_ci1(const GatherArgs& a, hipStream_t s) {
  const size_t lds = (size_t)((CI1_RB - 1) * a.S + (a.K - 1) * a.D + 1) * sizeof(float);
  const dim3 grid((a.T_out + CI1_RB - 1) / CI1_RB, a.B);
  if (a.K == 4) launch_gather_ci1_k<TX, TY, 4>(a, grid, lds, s);
  else launch_gather_ci1_k<TX, TY, 0>(a, grid, lds, s);
  VQA_LAUNCHED("gather_ci1_kernel");
  return VQA_OK;
}

static bool ci1_ok(const GatherArgs& a) {
  return a.C == 1 && a.wmode == W_DIRECT && (a.O == 32 || a.O == 64) && a.K <= CI1_KMAX &&
         !(a.flags & (VQA_POST_MASK | VQA_ADD_RESIDUAL)) &&
         (size_t)((CI1_RB - 1) * a.S + (a.K - 1) * a.D + 1) * sizeof(float) <= 64 * 1024;
}

GatherRoute gather_route(const GatherArgs& a, int dtype) {
  GatherRoute r{};
  if ((r.pvx = conv32_pvx(a, dtype, false))) {
    r.family = G_CONV32;
    return r;
  }
  r.m = mfma_plan(a, dtype);
  if (r.m.ok) {
    r.family = G_MFMA;
  } else if (ci1_ok(a)) {
    r.family = G_CI1;
  } else if (a.O <= 8 && (a.C == 32 || a.C == 64) && a.wmode != W_PAIR && a.K <= 4 && a.S <= 2 && a.D <= 64) {
    r.family = G_THINO;
  } else if ((a.C <= 8 || a.O <= 8) && (size_t)a.K * a.C * a.O * 4 <= 64 * 1024 &&
             (a.wmode != W_PAIR || (a.O / 2) % 8 == 0 || a.O % 8 != 0)) {
    r.family = G_THIN;
  } else {
    r.family = G_DIRECT;
  }
  return r;
}

// the shape checks of every gather conv (pointers apart)
int gather_check(const GatherArgs& a, int dtype) {
  VQA_ARG(dtype == VQA_F32 || dtype == VQA_BF16, "unknown dtype %d", dtype);
  VQA_ARG(a.B > 0 && a.T_in > 0 && a.T_out > 0 && a.C > 0 && a.O > 0 && a.K > 0 && a.S > 0 && a.D > 0,
          "non-positive shape");
  return VQA_OK;
}

int run_gather(const GatherArgs& a, int dtype, hipStream_t s) {
  const int rc = gather_check(a, dtype);
  if (rc != VQA_OK) return rc;
  VQA_ARG(a.x && a.w && a.y, "null tensor pointer");
  VQA_ARG(!(a.flags & VQA_POST_MASK) || a.mask, "VQA_POST_MASK without mask");
  VQA_ARG(!(a.flags & VQA_ADD_RESIDUAL) || a.resid, "VQA_ADD_RESIDUAL without residual");
  const GatherRoute r = gather_route(a, dtype);
  const bool xf = dtype == VQA_F32 || (a.flags & VQA_X_F32);
  const bool yf = dtype == VQA_F32 || (a.flags & VQA_Y_F32);
  if (r.family == G_CONV32)
    return dtype == VQA_BF16 ? launch_conv32<bf16, false>(a, r.pvx, s, nullptr)
                             : launch_conv32<float, false>(a, r.pvx, s, nullptr);
  if (r.family == G_MFMA)
    return dtype == VQA_BF16 ? launch_gather_mfma<bf16>(a, r.m, s) : launch_gather_mfma<float>(a, r.m, s);
  return dispatch_xy(xf, yf, [&](auto tx, auto ty) {
    typedef tag_t<decltype(tx)> TX;
    typedef tag_t<decltype(ty)> TY;
    switch (r.family) {
      case G_CI1: return launch_gather_ci1<TX, TY>(a, s);
      case G_THINO: return launch_gather_thinO<TX, TY>(a, s);
      case G_THIN: return launch_gather_thin<TX, TY>(a, s);
      default: {
        GatherArgs b = a;
        if (!xf && !yf) b.wbf16 = mfma_channels(a) ? 1 : 0;  // the all-bf16 conv: weights as the MFMA kernels stage them
        return launch_gather_direct<TX, TY>(b, s);
      }
    }
  });
}

int launch_conv32_fused(const GatherArgs& a, int pvx, int dtype, hipStream_t s, int* nwg) {
  return dtype == VQA_BF16 ? launch_conv32<bf16, true>(a, pvx, s, nwg) : launch_conv32<float, true>(a, pvx, s, nwg);
}

}  // namespace vqa
