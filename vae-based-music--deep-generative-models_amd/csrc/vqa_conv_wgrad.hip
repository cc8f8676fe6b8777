// vqa_conv_wgrad.hip — the conv weight-gradient kernels (vqa_conv.h has the formulation and the partial layout), the
// reducers that sum the per-workgroup fp32 partials in a fixed order, and the host plan run_wgrad launches from.
#include "vqa_conv.h"
#include "vqa_launch.h"
#include "vqa_mfma.h"

namespace vqa {

// Register-staged row loader (issue early, write late — cdna_hip_programming.md T14): chunk
// e = threadIdx.x + i*256 of a rows x C tile, 16 B each, PV chunks per thread held in VGPRs; chunks
// beyond 256*PV are staged synchronously by tail().
template <class T, int C, int PV>
struct RowStager {
  static constexpr int VEC = 16 / (int)sizeof(T), CPR = C / VEC;
  uint4 v[PV];
  unsigned ok;
  // branch-free issue (see TileRegs::load in vqa_conv_gather.hip); requires lo < hi (a non-empty row range)
  __device__ __forceinline__ void load(const T* Xi, int lo, int hi, int r0, int rows) {
    ok = 0u;
#pragma unroll
    for (int i = 0; i < PV; ++i) {
      const int e = threadIdx.x + i * 256;
      const int rr = e / CPR, q = e - rr * CPR, ti = r0 + rr;
      const bool val = e < rows * CPR && ti >= lo && ti < hi;
      const int tc = val ? ti : lo;
      v[i] = *((const uint4*)(Xi + (long long)tc * C) + (val ? q : 0));
      ok |= val ? (1u << i) : 0u;
    }
  }
  __device__ __forceinline__ void store(T* xl, int XS, int rows, bool relu) {
#pragma unroll
    for (int i = 0; i < PV; ++i) {
      const int e = threadIdx.x + i * 256;
      if (e < rows * CPR) {
        const int rr = e / CPR, q = e - rr * CPR;
        uint4 t = v[i];
        if (!(ok & (1u << i))) t = uint4{0u, 0u, 0u, 0u};
        if (relu) relu_bits<T>(t);
        *(uint4*)(xl + rr * XS + q * VEC) = t;
      }
    }
  }
  __device__ __forceinline__ void tail(T* xl, int XS, const T* Xi, int lo, int hi, int r0, int rows, bool relu) {
    for (int e = threadIdx.x + PV * 256; e < rows * CPR; e += 256) {
      const int rr = e / CPR, q = e - rr * CPR, ti = r0 + rr;
      uint4 t = {0u, 0u, 0u, 0u};
      if (ti >= lo && ti < hi) t = *((const uint4*)(Xi + (long long)ti * C) + q);
      if (relu) relu_bits<T>(t);
      *(uint4*)(xl + rr * XS + q * VEC) = t;
    }
  }
};

template <class T, int C, int O, int TT>
__global__ __launch_bounds__(256) void wgrad_mfma_kernel(WgradArgs a) {
  typedef Mfma<T> M;
  constexpr int XS = C + lds_pad<T>();
  constexpr int GS = O + lds_pad<T>();
  constexpr int CT = C / 16, OT = O / 16;
  constexpr int MAXTW = CT * OT;  // max tiles per wave (K <= 4 taps over 4 waves)
  constexpr int KT = (int)sizeof(T) == 2 ? 32 : 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* gl = (T*)smem;
  T* xl = gl + TT * GS;
  __shared__ float red[256];

  const int n = blockIdx.y, ch = blockIdx.x;
  const int tbeg = ch * a.CH, tend = min(a.T_out, tbeg + a.CH);
  const int rows_in = (TT - 1) * a.S + (a.K - 1) * a.D + 1;
  const int ntile = a.K * CT * OT;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;

  f32x4 acc[MAXTW];
#pragma unroll
  for (int i = 0; i < MAXTW; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dbacc = 0.f;
  const bool db_x = a.flags & WG_DB_FROM_X;
  const int NB = db_x ? C : O;
  const int dbo = threadIdx.x % NB, dbr = threadIdx.x / NB, dbstep = 256 / NB;

  const bool relu = a.flags & VQA_PRE_RELU;
  const T* Gi = (const T*)a.g + (long long)n * a.T_out * O;
  const T* Xi = (const T*)a.x + (long long)n * a.T_in * C;
  RowStager<T, O, 4> sg;
  // input chunks per thread: the model's input spans without the tail loop (whose loads were waited for one by one
  // before every sub-tile's store): bf16 C = 32 stride 2 K = 4 (258 rows x 4 chunks) -> 5; C = 64 stride 1 K = 3
  // (130 x 8) and stride 2 K = 4 (258 x 8) -> 9
  RowStager<T, C, sizeof(T) == 2 ? (C == 32 ? 5 : (C == 64 ? 9 : 4)) : 4> sx;
  if (tbeg < tend) {
    const int nrows = min(TT, tend - tbeg);
    sg.load(Gi, tbeg, tbeg + nrows, tbeg, TT);
    sx.load(Xi, 0, a.T_in, tbeg * a.S - a.P, rows_in);
    sg.store(gl, GS, TT, false);
    sg.tail(gl, GS, Gi, tbeg, tbeg + nrows, tbeg, TT, false);
    sx.store(xl, XS, rows_in, relu);
    sx.tail(xl, XS, Xi, 0, a.T_in, tbeg * a.S - a.P, rows_in, relu);
  }
  __syncthreads();
  for (int t0 = tbeg; t0 < tend; t0 += TT) {
    const int nrows = min(TT, tend - t0);
    const int t1 = t0 + TT;
    const bool has_next = t1 < tend;
    const int nrows1 = has_next ? min(TT, tend - t1) : 0;
    if (has_next) {  // prefetch the next sub-tile while this one is reduced
      sg.load(Gi, t1, t1 + nrows1, t1, TT);
      sx.load(Xi, 0, a.T_in, t1 * a.S - a.P, rows_in);
    }
    if (db_x) {
      for (int r = a.P + dbr; r < a.P + nrows * a.S; r += dbstep) dbacc += (float)xl[r * XS + dbo];
    } else {
      for (int r = dbr; r < nrows; r += dbstep) dbacc += (float)gl[r * GS + dbo];
    }
#pragma unroll
    for (int ti = 0; ti < MAXTW; ++ti) {
      const int tile = wave + 4 * ti;
      if (tile < ntile) {
        const int ot = tile % OT, rest = tile / OT, ct = rest % CT, k = rest / CT;
        // K = output rows: transposed LDS reads of both operands (same even/odd K order)
        const T* xp = xl + (size_t)(k * a.D) * XS + ct * 16;
        const T* gp = gl + ot * 16;
        f32x4 c = acc[ti];
#pragma unroll
        for (int kk = 0; kk < TT; kk += KT) {
          const typename M::frag af = M::rows_eo(xp + (size_t)(kk * a.S) * XS, a.S * XS);
          const typename M::frag bf = M::rows_eo(gp + (size_t)kk * GS, GS);
          c = M::mma(af, bf, c);
        }
        acc[ti] = c;
      }
    }
    __syncthreads();
    if (has_next) {
      sg.store(gl, GS, TT, false);
      sg.tail(gl, GS, Gi, t1, t1 + nrows1, t1, TT, false);
      sx.store(xl, XS, rows_in, relu);
      sx.tail(xl, XS, Xi, 0, a.T_in, t1 * a.S - a.P, rows_in, relu);
    }
    __syncthreads();
  }

  float* out = a.ws + (size_t)(n * a.nchunk + ch) * (size_t)(a.K * C * O + NB);
#pragma unroll
  for (int ti = 0; ti < MAXTW; ++ti) {
    const int tile = wave + 4 * ti;
    if (tile < ntile) {
      const int ot = tile % OT, rest = tile / OT, ct = rest % CT, k = rest / CT;
      const int o = ot * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = ct * 16 + 4 * (lane >> 4) + r;
        out[((size_t)k * C + c) * O + o] = acc[ti][r];
      }
    }
  }
  red[threadIdx.x] = dbacc;
  __syncthreads();
  if (threadIdx.x < NB) {
    float s = 0.f;
    for (int r = 0; r < dbstep; ++r) s += red[r * NB + threadIdx.x];
    out[a.K * C * O + threadIdx.x] = s;
  }
}

// ------------------------------------------------------------------------------------------------
// Thin weight gradients for the 1-channel waveform layers. Threads = RL row lanes x VL lanes of 8
// consecutive channels along the WIDE side; 16-byte loads along it; LDS reduction over row lanes.
//   WIDE_X: C % 8 == 0, O <= 2 (decoder output conv, C=64 -> O=1)
//   WIDE_G: O % 8 == 0, C <= 2 (first encoder conv, C=1 -> O=32)

// buffer loads converting to fp32 (an out-of-range offset reads zeros)
template <class T> __device__ __forceinline__ float ld1_buf(__amdgpu_buffer_rsrc_t r, int off);
template <> __device__ __forceinline__ float ld1_buf<float>(__amdgpu_buffer_rsrc_t r, int off) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0));
}
template <> __device__ __forceinline__ float ld1_buf<bf16>(__amdgpu_buffer_rsrc_t r, int off) {
  return __uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b16(r, off, 0, 0) << 16);
}
template <class T> __device__ __forceinline__ void ld8_buf(__amdgpu_buffer_rsrc_t r, int off, float* v);
template <> __device__ __forceinline__ void ld8_buf<bf16>(__amdgpu_buffer_rsrc_t r, int off, float* v) {
  const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = __uint_as_float(w[i] << 16);
    v[2 * i + 1] = __uint_as_float(w[i] & 0xFFFF0000u);
  }
}
template <> __device__ __forceinline__ void ld8_buf<float>(__amdgpu_buffer_rsrc_t r, int off, float* v) {
  const u32x4 a = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
  const u32x4 b = __builtin_amdgcn_raw_buffer_load_b128(r, off + 16, 0, 0);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[i] = __uint_as_float(a[i]);
    v[i + 4] = __uint_as_float(b[i]);
  }
}

// NM: the narrow side's width bound (1 for the model's 1-channel ends: half the accumulators and tap registers of
// NM = 2, 29.4 vs 33.6 us for the first encoder conv at cfg2, the same sums in the same order)
template <class TX, class TG, bool WIDE_X, int NM>
__global__ __launch_bounds__(256) void wgrad_thin_kernel(WgradArgs a) {
  constexpr int KM = 4, U = 8;  // max taps, rows in flight per thread
  const int W = WIDE_X ? a.C : a.O;
  const int NN = WIDE_X ? a.O : a.C;
  const int VL = W / 8, RL = 256 / VL;
  const int v = threadIdx.x % VL, rl = threadIdx.x / VL;
  const int n = blockIdx.y, ch = blockIdx.x;
  const int tbeg = ch * a.CH, tend = min(a.T_out, tbeg + a.CH);
  const bool relu = a.flags & VQA_PRE_RELU;
  // the item's rows as buffer resources (host-checked: an item is < 2^30 bytes)
  const unsigned xbytes = (unsigned)a.T_in * a.C * (unsigned)sizeof(TX), gbytes = (unsigned)a.T_out * a.O * (unsigned)sizeof(TG);
  const __amdgpu_buffer_rsrc_t rx = item_rsrc(a.x, (long long)n * xbytes, xbytes);
  const __amdgpu_buffer_rsrc_t rg = item_rsrc(a.g, (long long)n * gbytes, gbytes);
  float acc[KM][NM][8];
  float bacc[8];
#pragma unroll
  for (int k = 0; k < KM; ++k)
#pragma unroll
    for (int i = 0; i < NM; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[k][i][j] = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) bacc[j] = 0.f;
  if (rl < RL) {
    // U rows per iteration, all loads issued before the FMAs (memory-level parallelism)
    for (int t = tbeg + rl; t < tend; t += U * RL) {
      float gv[U][WIDE_X ? NM : 8];
      float xv[U][KM][WIDE_X ? 8 : NM];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        // every load issued unconditionally: rows past the chunk and taps outside the item get an out-of-range
        // buffer offset (kOOB), which reads zeros (a load in a branch was waited for right there: 8 serial round
        // trips per iteration, 33 us at the first conv)
        const int tt = t + u * RL;
        const bool okr = tt < tend;
        const int goff = okr ? (tt * a.O + (WIDE_X ? 0 : v * 8)) * (int)sizeof(TG) : kOOB;
        if (WIDE_X) {
#pragma unroll
          for (int i = 0; i < NM; ++i) gv[u][i] = ld1_buf<TG>(rg, i < NN ? goff + i * (int)sizeof(TG) : kOOB);
        } else {
          ld8_buf<TG>(rg, goff, gv[u]);
        }
#pragma unroll
        for (int k = 0; k < KM; ++k) {
          const int ti = tt * a.S + k * a.D - a.P;
          const bool ok = okr && k < a.K && ti >= 0 && ti < a.T_in;
          const int xoff = ok ? (ti * a.C + (WIDE_X ? v * 8 : 0)) * (int)sizeof(TX) : kOOB;
          if (WIDE_X) {
            ld8_buf<TX>(rx, xoff, xv[u][k]);
          } else {
#pragma unroll
            for (int i = 0; i < NM; ++i) xv[u][k][i] = ld1_buf<TX>(rx, i < NN ? xoff + i * (int)sizeof(TX) : kOOB);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (WIDE_X) {
          if (v == 0)
#pragma unroll
            for (int i = 0; i < NM; ++i) bacc[i] += gv[u][i];
#pragma unroll
          for (int k = 0; k < KM; ++k)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const float x = relu ? fmaxf(xv[u][k][j], 0.f) : xv[u][k][j];
#pragma unroll
              for (int i = 0; i < NM; ++i) acc[k][i][j] += x * gv[u][i];
            }
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) bacc[j] += gv[u][j];
#pragma unroll
          for (int k = 0; k < KM; ++k)
#pragma unroll
            for (int i = 0; i < NM; ++i) {
              const float x = relu ? fmaxf(xv[u][k][i], 0.f) : xv[u][k][i];
#pragma unroll
              for (int j = 0; j < 8; ++j) acc[k][i][j] += x * gv[u][j];
            }
        }
      }
    }
  }
  // reduce over row lanes: per thread KM*NM*8 + 8 values
  constexpr int PER = KM * NM * 8 + 8;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* red = (float*)smem;  // [256][PER]
  {
    float* r = red + threadIdx.x * PER;
    int q = 0;
#pragma unroll
    for (int k = 0; k < KM; ++k)
#pragma unroll
      for (int i = 0; i < NM; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) r[q++] = acc[k][i][j];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[q++] = bacc[j];
  }
  __syncthreads();
  const int KCO = a.K * a.C * a.O;
  float* out = a.ws + (size_t)(n * a.nchunk + ch) * (size_t)(KCO + a.nb);
  for (int e = threadIdx.x; e < KCO + a.nb; e += 256) {
    int vv, q;
    if (e < KCO) {
      const int o = e % a.O, c = (e / a.O) % a.C, k = e / (a.O * a.C);
      const int wide = WIDE_X ? c : o, narrow = WIDE_X ? o : c;
      vv = wide / 8;
      q = (k * NM + narrow) * 8 + (wide % 8);
    } else {
      const int o = e - KCO;
      vv = WIDE_X ? 0 : o / 8;
      q = KM * NM * 8 + (WIDE_X ? o : o % 8);
    }
    float sum = 0.f;
    for (int r = 0; r < RL; ++r) sum += red[(r * VL + vv) * PER + q];
    out[e] = sum;
  }
}

// Generic VALU weight gradient (small K*C*O: the 1-channel layers). Same partial layout.
template <class TX, class TG, int TT>
__global__ __launch_bounds__(256) void wgrad_direct_kernel(WgradArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* gl = (float*)smem;           // [TT][O]
  float* xl = gl + TT * a.O;          // [rows_in][C]
  constexpr int EPT = 16;
  const int n = blockIdx.y, ch = blockIdx.x;
  const int tbeg = ch * a.CH, tend = min(a.T_out, tbeg + a.CH);
  const int rows_in = (TT - 1) * a.S + (a.K - 1) * a.D + 1;
  const int E = a.K * a.C * a.O;
  const int e0 = blockIdx.z * EPT * 256;  // this slice's weight elements [e0, e0 + 4096) (gridDim.z slices)
  const bool relu = a.flags & VQA_PRE_RELU;
  float acc[EPT];
#pragma unroll
  for (int i = 0; i < EPT; ++i) acc[i] = 0.f;
  float dbacc = 0.f;
  for (int t0 = tbeg; t0 < tend; t0 += TT) {
    const int nrows = min(TT, tend - t0);
    for (int e = threadIdx.x; e < TT * a.O; e += blockDim.x) {
      const int r = e / a.O, o = e - r * a.O;
      gl[e] = r < nrows ? ld((const TG*)a.g + ((long long)n * a.T_out + t0 + r) * a.O + o) : 0.f;
    }
    for (int e = threadIdx.x; e < rows_in * a.C; e += blockDim.x) {
      const int r = e / a.C, c = e - r * a.C;
      const int ti = t0 * a.S - a.P + r;
      float v = (ti >= 0 && ti < a.T_in) ? ld((const TX*)a.x + ((long long)n * a.T_in + ti) * a.C + c) : 0.f;
      xl[e] = relu ? fmaxf(v, 0.f) : v;
    }
    __syncthreads();
    if (blockIdx.z == 0) {
      if (a.flags & WG_DB_FROM_X) {
        if (threadIdx.x < a.C)
          for (int r = a.P; r < a.P + nrows * a.S; ++r) dbacc += xl[r * a.C + threadIdx.x];
      } else if (threadIdx.x < a.O) {
        for (int r = 0; r < nrows; ++r) dbacc += gl[r * a.O + threadIdx.x];
      }
    }
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      const int e = e0 + threadIdx.x + i * 256;
      if (e < E) {
        const int o = e % a.O, c = (e / a.O) % a.C, k = e / (a.O * a.C);
        float s = acc[i];
        for (int r = 0; r < nrows; ++r) s += xl[(r * a.S + k * a.D) * a.C + c] * gl[r * a.O + o];
        acc[i] = s;
      }
    }
    __syncthreads();
  }
  float* out = a.ws + (size_t)(n * a.nchunk + ch) * (size_t)(E + a.nb);
#pragma unroll
  for (int i = 0; i < EPT; ++i) {
    const int e = e0 + threadIdx.x + i * 256;
    if (e < E) out[e] = acc[i];
  }
  if (blockIdx.z == 0 && threadIdx.x < a.nb) out[E + threadIdx.x] = dbacc;
}

// out1[e] = sum_p ws[p*E + e] for e < E1, out2[e - E1] likewise for e >= E1. Block = 16 elements x 16 part
// groups (64-byte row segments); each thread keeps 8 independent partial sums (memory-level parallelism);
// the sums and then the groups are combined in a fixed order, so the result is deterministic.
constexpr int kRedCols = 16;
__device__ __forceinline__ float reduce_col16(const float* ws, int nparts, int E, int e, float (*red)[kRedCols]) {
  const int el = threadIdx.x & (kRedCols - 1), grp = threadIdx.x / kRedCols;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (e < E) {
    int p = grp;
    for (; p + 7 * 16 < nparts; p += 8 * 16)
#pragma unroll
      for (int u = 0; u < 8; ++u) s[u] += ws[(size_t)(p + 16 * u) * E + e];
    for (; p < nparts; p += 16) s[0] += ws[(size_t)p * E + e];
  }
  red[grp][el] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  __syncthreads();
  float t = 0.f;
  if (grp == 0)
    for (int g = 0; g < 16; ++g) t += red[g][el];
  return t;
}

// Wide form (rows whose length and base keep float4 alignment): block = 256 elements (64 lanes x 4) of every
// partial row, each wave reading 1 KB of one row per load (4 rows at a time over the 4 waves, 8 rows in flight
// per wave); the 8 per-thread sums, then the 4 waves, are combined in a fixed order: deterministic.
constexpr int kRedCols256 = 256;
__device__ __forceinline__ f32x4 reduce_col256(const float* ws, int nparts, int E, int e, f32x4 (*red)[64]) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  f32x4 s[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) s[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (e < E) {
    int p = wave;
    for (; p + 4 * 7 < nparts; p += 4 * 8)
#pragma unroll
      for (int u = 0; u < 8; ++u) s[u] += *(const f32x4*)(ws + (size_t)(p + 4 * u) * E + e);
    for (; p < nparts; p += 4) s[0] += *(const f32x4*)(ws + (size_t)p * E + e);
  }
  red[wave][lane] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  __syncthreads();
  f32x4 t = {0.f, 0.f, 0.f, 0.f};
  if (wave == 0) t = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
  return t;
}

static bool desc_vec4(const vqa_partials_desc& d) {
  return d.n % 4 == 0 && ((uintptr_t)d.partials & 15) == 0;
}

__global__ __launch_bounds__(256) void reduce_partials_kernel(const float* ws, int nparts, int E, int E1,
                                                             float* out1, float* out2) {
  __shared__ float red[16][kRedCols];
  const int e = blockIdx.x * kRedCols + (threadIdx.x & (kRedCols - 1));
  const float s = reduce_col16(ws, nparts, E, e, red);
  if (threadIdx.x < kRedCols && e < E) {
    if (e < E1) {
      if (out1) out1[e] = s;
    } else if (out2) {
      out2[e - E1] = s;
    }
  }
}

// Batched form: one launch reduces up to kMaxDescs layers; block b belongs to the descriptor whose
// [start, start + ceil(n/16)) range contains it. Same fixed summation order as reduce_partials_kernel.
constexpr int kMaxDescs = 48;
struct ReduceBatch {
  vqa_partials_desc d[kMaxDescs];
  int start[kMaxDescs + 1];
  int vec4[kMaxDescs];
  int count;
};

__global__ __launch_bounds__(256) void reduce_partials_batched_kernel(ReduceBatch rb) {
  __shared__ f32x4 red4[16][16];
  int i = 0;
  while (i + 1 < rb.count && (int)blockIdx.x >= rb.start[i + 1]) ++i;
  const vqa_partials_desc& d = rb.d[i];
  if (rb.vec4[i]) {
#ifdef VQA_REDUCE_COL64  // A/B only: the round-3 layout (64 columns x 16 row groups per block)
    const int e = ((int)blockIdx.x - rb.start[i]) * 64 + 4 * (threadIdx.x & 15);
    f32x4 s;
    {
      const int el = threadIdx.x & 15, grp = threadIdx.x >> 4;
      f32x4 t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (e < d.n) {
        int p = grp;
        for (; p + 7 * 16 < d.nparts; p += 8 * 16)
#pragma unroll
          for (int u = 0; u < 8; ++u) t[u] += *(const f32x4*)(d.partials + (size_t)(p + 16 * u) * d.n + e);
        for (; p < d.nparts; p += 16) t[0] += *(const f32x4*)(d.partials + (size_t)p * d.n + e);
      }
      red4[grp][el] = ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
      __syncthreads();
      s = f32x4{0.f, 0.f, 0.f, 0.f};
      if (grp == 0)
        for (int g = 0; g < 16; ++g) s += red4[g][el];
    }
    if (threadIdx.x < 16 && e < d.n) {
#else
    const int e = ((int)blockIdx.x - rb.start[i]) * kRedCols256 + 4 * (threadIdx.x & 63);
    const f32x4 s = reduce_col256(d.partials, d.nparts, d.n, e, (f32x4(*)[64])red4);
    if (threadIdx.x < 64 && e < d.n) {
#endif
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int eq = e + q;
        if (eq < d.n_w) {
          if (d.dw) d.dw[eq] = s[q];
        } else if (d.db) {
          d.db[eq - d.n_w] = s[q];
        }
      }
    }
    return;
  }
  float(*red)[kRedCols] = (float(*)[kRedCols])red4;
  const int e = ((int)blockIdx.x - rb.start[i]) * kRedCols + (threadIdx.x & (kRedCols - 1));
  const float s = reduce_col16(d.partials, d.nparts, d.n, e, red);
  if (threadIdx.x < kRedCols && e < d.n) {
    if (e < d.n_w) {
      if (d.dw) d.dw[e] = s;
    } else if (d.db) {
      d.db[e - d.n_w] = s;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side
static WgradPlan plan_wgrad(int dtype, int B, int T_in, int T_out, int C, int O, int K, int S, int D, int flags) {
  WgradPlan p{};
  const bool anyf32 = (flags & (VQA_X_F32 | VQA_Y_F32)) != 0;
  const size_t esz = dtype == VQA_BF16 ? 2 : 4;
  p.nb = (flags & WG_DB_FROM_X) ? C : O;
  // the thin kernels address an item's rows through 32-bit buffer offsets
  const bool thin_fits = (long long)T_in * C * 4 < (1ll << 30) && (long long)T_out * O * 4 < (1ll << 30);
  if (!anyf32 && (C == 32 || C == 64) && (O == 32 || O == 64) && K <= 4) {
    p.kind = WG_MFMA;
    p.TT = dtype == VQA_BF16 ? 128 : 64;
    const int rows_in = (p.TT - 1) * S + (K - 1) * D + 1;
    p.lds = ((size_t)p.TT * (O + 16 / esz) + (size_t)rows_in * (C + 16 / esz)) * esz;
    if (p.lds > 150 * 1024) {
      p.TT = 64;
      const int r2 = (p.TT - 1) * S + (K - 1) * D + 1;
      p.lds = ((size_t)p.TT * (O + 16 / esz) + (size_t)r2 * (C + 16 / esz)) * esz;
    }
  } else if (K <= 4 && C % 8 == 0 && C <= 256 && O <= 2 && !(flags & WG_DB_FROM_X) && thin_fits) {
    p.kind = WG_THIN_X;
    p.TT = 64;
    p.lds = (size_t)256 * (4 * 2 * 8 + 8) * sizeof(float);
  } else if (K <= 4 && O % 8 == 0 && O <= 256 && C <= 2 && !(flags & WG_DB_FROM_X) && thin_fits) {
    p.kind = WG_THIN_G;
    p.TT = 64;
    p.lds = (size_t)256 * (4 * 2 * 8 + 8) * sizeof(float);
  } else {
    p.kind = WG_DIRECT;
    p.TT = 64;
    const int rows_in = (p.TT - 1) * S + (K - 1) * D + 1;
    p.lds = ((size_t)p.TT * O + (size_t)rows_in * C) * 4;
  }
  // ~512 workgroups (two per CU): each streams its rows once (4 rows in flight per thread in the thin
  // kinds) and the partials stay small
  const long long target = 512;
  const long long per_item = (target + B - 1) / B;
  int ch = (int)((T_out + per_item - 1) / per_item);
  ch = ((ch + p.TT - 1) / p.TT) * p.TT;
  if (ch < p.TT) ch = p.TT;
  p.CH = ch;
  p.nchunk = (T_out + ch - 1) / ch;
  p.nwg = p.nchunk * B;
  p.E = K * C * O + p.nb;
  p.ws_bytes = (size_t)p.nwg * p.E * sizeof(float);
  return p;
}

// The plan of a weight gradient and the checks it must pass before anything is launched (no HIP call): what
// run_wgrad launches from and vqa_conv1d_route reports from.
int wgrad_route(WgradPlan* out, int dtype, int B, int T_in, int T_out, int C, int O, int K, int S, int D, int flags) {
  VQA_ARG(dtype == VQA_F32 || dtype == VQA_BF16, "unknown dtype %d", dtype);
  VQA_ARG(B > 0 && T_in > 0 && T_out > 0 && C > 0 && O > 0 && K > 0 && S > 0 && D > 0, "non-positive shape");
  const WgradPlan p = plan_wgrad(dtype, B, T_in, T_out, C, O, K, S, D, flags);
  *out = p;
  VQA_REQUIRE(p.lds <= 150 * 1024, VQA_E_UNSUPPORTED, "wgrad: LDS tile too large (%zu B)", p.lds);
  VQA_REQUIRE(p.kind != WG_DIRECT || K * C * O <= 16 * 256 * 64, VQA_E_UNSUPPORTED,
              "wgrad: generic path limited to K*C*O<=262144");
  VQA_REQUIRE(p.nb <= 256 && 256 % p.nb == 0, VQA_E_UNSUPPORTED, "wgrad: bias width must divide 256");
  return VQA_OK;
}

template <class T, int C, int O, int TT>
static int launch_wgrad_mfma_t(const WgradArgs& a, const WgradPlan& p, hipStream_t s) {
  const int rc = raise_dyn_lds((const void*)wgrad_mfma_kernel<T, C, O, TT>, p.lds, "wgrad_mfma_kernel");
  if (rc != VQA_OK) return rc;
  hipLaunchKernelGGL((wgrad_mfma_kernel<T, C, O, TT>), dim3(p.nchunk, a.B), dim3(256), p.lds, s, a);
  VQA_LAUNCHED("wgrad_mfma_kernel");
  return VQA_OK;
}

template <class T, int C, int O>
static int launch_wgrad_mfma_co(const WgradArgs& a, const WgradPlan& p, hipStream_t s) {
  if (p.TT == 128) return launch_wgrad_mfma_t<T, C, O, 128>(a, p, s);
  return launch_wgrad_mfma_t<T, C, O, 64>(a, p, s);
}

template <class T>
static int launch_wgrad_mfma(const WgradArgs& a, const WgradPlan& p, hipStream_t s) {
  if (a.C == 32 && a.O == 32) return launch_wgrad_mfma_co<T, 32, 32>(a, p, s);
  if (a.C == 32 && a.O == 64) return launch_wgrad_mfma_co<T, 32, 64>(a, p, s);
  if (a.C == 64 && a.O == 32) return launch_wgrad_mfma_co<T, 64, 32>(a, p, s);
  if (a.C == 64 && a.O == 64) return launch_wgrad_mfma_co<T, 64, 64>(a, p, s);
  vqa::set_error("wgrad: no MFMA tile for C=%d O=%d", a.C, a.O);
  return VQA_E_UNSUPPORTED;
}

template <class TX, class TG>
static int launch_wgrad_direct(const WgradArgs& a, const WgradPlan& p, hipStream_t s) {
  const int rc = raise_dyn_lds((const void*)wgrad_direct_kernel<TX, TG, 64>, p.lds, "wgrad_direct_kernel");
  if (rc != VQA_OK) return rc;
  const unsigned slices = (unsigned)((a.K * a.C * a.O + 4095) / 4096);  // 16 weight elements per thread per slice
  hipLaunchKernelGGL((wgrad_direct_kernel<TX, TG, 64>), dim3(p.nchunk, a.B, slices), dim3(256), p.lds, s, a);
  VQA_LAUNCHED("wgrad_direct_kernel");
  return VQA_OK;
}

template <class TX, class TG, bool WX, int NM>
static int launch_wgrad_thin_nm(const WgradArgs& a, const WgradPlan& p, hipStream_t s) {
  const int rc = raise_dyn_lds((const void*)wgrad_thin_kernel<TX, TG, WX, NM>, p.lds, "wgrad_thin_kernel");
  if (rc != VQA_OK) return rc;
  hipLaunchKernelGGL((wgrad_thin_kernel<TX, TG, WX, NM>), dim3(p.nchunk, a.B), dim3(256), p.lds, s, a);
  VQA_LAUNCHED("wgrad_thin_kernel");
  return VQA_OK;
}

template <class TX, class TG, bool WX>
static int launch_wgrad_thin(const WgradArgs& a, const WgradPlan& p, hipStream_t s) {
  return (WX ? a.O : a.C) == 1 ? launch_wgrad_thin_nm<TX, TG, WX, 1>(a, p, s) : launch_wgrad_thin_nm<TX, TG, WX, 2>(a, p, s);
}

int reduce_partials(const float* ws, int nparts, int E, int n_w, float* dw, float* db, hipStream_t s) {
  hipLaunchKernelGGL(reduce_partials_kernel, dim3((E + kRedCols - 1) / kRedCols), dim3(256), 0, s, ws, nparts, E, n_w,
                     dw, db);
  VQA_LAUNCHED("reduce_partials_kernel");
  return VQA_OK;
}

int run_wgrad(const void* x, const void* g, float* dw, float* db, int B, int T_in, int T_out, int C, int O, int K,
              int S, int D, int P, int flags, int dtype, void* ws, size_t ws_bytes, hipStream_t s,
              vqa_partials_desc* defer) {
  VQA_ARG(x && g && dw, "null tensor pointer");
  WgradPlan p{};
  int rc = wgrad_route(&p, dtype, B, T_in, T_out, C, O, K, S, D, flags);
  if (rc != VQA_OK) return rc;
  VQA_ARG(ws && ws_bytes >= p.ws_bytes, "workspace too small: need %zu bytes, got %zu", p.ws_bytes, ws_bytes);
  WgradArgs a{x, g, (float*)ws, B, T_in, T_out, C, O, K, S, D, P, p.CH, p.nchunk, flags, p.nb};
  const bool xf = dtype == VQA_F32 || (flags & VQA_X_F32);
  const bool gf = dtype == VQA_F32 || (flags & VQA_Y_F32);
  if (p.kind == WG_MFMA) {
    rc = dtype == VQA_BF16 ? launch_wgrad_mfma<bf16>(a, p, s) : launch_wgrad_mfma<float>(a, p, s);
  } else {
    rc = dispatch_xy(xf, gf, [&](auto tx, auto tg) {
      typedef tag_t<decltype(tx)> TX;
      typedef tag_t<decltype(tg)> TG;
      if (p.kind == WG_THIN_X) return launch_wgrad_thin<TX, TG, true>(a, p, s);
      if (p.kind == WG_THIN_G) return launch_wgrad_thin<TX, TG, false>(a, p, s);
      return launch_wgrad_direct<TX, TG>(a, p, s);
    });
  }
  if (rc != VQA_OK) return rc;
  const int KCO = K * C * O;
  if (defer) {
    *defer = vqa_partials_desc{(const float*)ws, dw, db, p.nwg, p.E, KCO, 0};
    return VQA_OK;
  }
  return reduce_partials((const float*)ws, p.nwg, p.E, KCO, dw, db, s);
}

size_t wgrad_ws(int dtype, int B, int T_in, int T_out, int C, int O, int K, int S, int D, int flags) {
  if (B < 1 || T_in < 1 || T_out < 1 || C < 1 || O < 1 || K < 1 || S < 1 || D < 1) return 0;  // no such conv
  return plan_wgrad(dtype, B, T_in, T_out, C, O, K, S, D, flags).ws_bytes;
}

}  // namespace vqa

using namespace vqa;

extern "C" int vqa_reduce_partials(const vqa_partials_desc* descs, int count, vqa_stream_t stream) {
  VQA_ARG(count >= 0 && (count == 0 || descs), "reduce_partials: bad descriptor list");
  for (int base = 0; base < count; base += kMaxDescs) {
    ReduceBatch rb{};
    rb.count = count - base < kMaxDescs ? count - base : kMaxDescs;
    int blocks = 0;
    for (int i = 0; i < rb.count; ++i) {
      const vqa_partials_desc& d = descs[base + i];
      VQA_ARG(d.partials && d.n > 0 && d.nparts > 0 && d.n_w <= d.n, "reduce_partials: bad descriptor %d", base + i);
      rb.d[i] = d;
      rb.start[i] = blocks;
      rb.vec4[i] = desc_vec4(d) ? 1 : 0;
#ifdef VQA_REDUCE_COL64
      blocks += rb.vec4[i] ? (d.n + 63) / 64 : (d.n + kRedCols - 1) / kRedCols;
#else
      blocks += rb.vec4[i] ? (d.n + kRedCols256 - 1) / kRedCols256 : (d.n + kRedCols - 1) / kRedCols;
#endif
    }
    rb.start[rb.count] = blocks;
    hipLaunchKernelGGL(reduce_partials_batched_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, rb);
    VQA_LAUNCHED("reduce_partials_batched_kernel");
  }
  return VQA_OK;
}
