// vqa_prior_decode.hip — the prior's autoregressive decode (gfx950): one persistent workgroup per sample, with
// the prime, temperature, top-k and nucleus (top-p) selection.
//
// Replaces (reference file:line):
//   src/autoregressive/autoregressive_fmha.py:162-240    sample (Gumbel-max per step)      -> vqa_prior_decode
#include "vqa_prior.h"

namespace vqa {

// ---------------------------------------------------------------------------------------------------
// Autoregressive decode (autoregressive_fmha.py:162-240 sample()): the reference re-runs the whole model on
// the prefix at every step; here ONE persistent workgroup per sample walks the steps with a key/value cache
// (the factorized attention of position i only needs keys <= i, keys of the same column, or the previous
// block) and keeps the causal conv's last two LayerNorm outputs per layer in LDS. Per step: embedding, the
// depth residual-attention blocks, the output head, z = logits + Gumbel(seed, sample, step, bin) and
// next token = argmax z (RelaxedOneHotCategorical(1).sample() then argmax). fp32 throughout, weights fp32
// from L2. Optional: forced input tokens (teacher-forced check) and per-step logits output.
// A prime (vqa_prior_decode_primed) gives the first prime_len next-input tokens: those steps do everything up to
// the output head (the caches and the LayerNorm ring must hold them) and run the head only when the logits are
// asked for. The noise stays keyed by the absolute step, so priming a decode with its own first tokens
// reproduces the rest bit for bit. kPrimed = true is the instantiation that knows the prime; without one the
// step loop is the unprimed decode's. kFilter = true is the instantiation with a temperature and / or top-k
// (score = logit / temperature + G over the bins whose logit is >= the k-th largest of the row); the default
// (temperature 1, top-k off) runs kFilter = false, whose arithmetic is the unfiltered decode's. kFilter = 2
// (vqa_prior_decode_filtered with top_p < 1 or a `kept` output) is kFilter = 1 plus the nucleus threshold
// (dec_nucleus_threshold) and the count of the bins that took part in the draw. kFilter = 3
// (vqa_prior_decode_scored with a log-probability output) is kFilter = 2 plus the two log-sums of dec_score_max /
// dec_logprob; with both outputs NULL the host launches 0, 1 or 2 as before.
constexpr int kDecMaxLayers = 8;
constexpr int kDecW = 128;   // model width
constexpr int kDecAW = 32;   // attention width (m_attn 0.25)
constexpr int kDecMaxL = 2048;
// Softmax scratch of the decode kernel: heads rows of `scs` floats in one flat LDS array. A layer scores at most
// max(l, blocks) keys per head (row: p + 1 <= l; column: b + 1 <= blocks; previous row: l), so scs = max(l, blocks)
// and vqa_prior_decode accepts only heads * scs <= kDecScoreFloats: every sc[h * scs + idx] with h < heads and
// idx < cnt <= scs is then below heads * scs <= kDecScoreFloats. (2 heads of 2048-token blocks fill it; the
// kernel's other static LDS leaves no room for more.)
constexpr int kDecScoreFloats = VQA_DECODE_SCORE_FLOATS;
static_assert(kDecScoreFloats == 2 * kDecMaxL, "decode score scratch: 2 heads of kDecMaxL keys");

struct DecLayer {
  const float *ln1g, *ln1b, *qkvw, *qkvb, *qw, *qb, *kw, *kb, *vw, *vb, *ow, *ob, *pw, *pb, *ln2g, *ln2b, *mw, *mb;
  int type;
  // composed once per decode (prior_decode_prep_kernel): the causal conv followed by the query/key/value
  // EinsumDense (one 384 x 96 map straight to the heads) and the output EinsumDense followed by proj (32 x 128)
  float *cw, *cb, *opw, *opb;
};

struct DecArgs {
  DecLayer L[kDecMaxLayers];
  const float *emb, *pos, *hw, *hb;
  const float* ycond;     // (N, W) or null
  const float* xcond;     // (N, T, W) fp32 or null
  const int64_t* forced;  // (N, steps + 1) or null
  const int64_t* prime;   // (N, prime_len) or null: tokens[n][j] = prime[n][j - 1] for 1 <= j <= prime_len
  float* logits;          // (N, steps, bins) or null
  int64_t* tokens;        // (N, steps + 1)
  float* kc;              // (N, depth, T, 32) key cache
  float* vc;              // (N, depth, T, 32) value cache
  int N, steps, T, depth, H, l, bins, ldo;  // ldo: head weight row stride (>= bins, % 4 == 0)
  int scs;                // row stride of the score scratch: max(l, T / l); H * scs <= kDecScoreFloats
  long long start;
  unsigned long long seed;
  float scale, emb_scale, eps;
  int prime_len;          // 0 <= prime_len <= steps (0 without a prime)
  int topk;               // 0: off, else 1 <= topk < bins (kFilter only)
  float temp;             // temperature, finite and > 0 (kFilter only)
  float topp;             // nucleus mass, 0 < topp <= 1, >= 1: off (kFilter = 2 only)
  int* kept;              // (N, steps) bins that took part in each draw, or null (kFilter >= 2 only)
  float* logp_model;      // (N, steps) log-probability of the written token under the model, or null (kFilter = 3)
  float* logp_draw;       // (N, steps) the same under the distribution the draw was made from, or null (kFilter = 3)
};

// y[o] = b[o] + sum_k x[k] W[k][o] (W row-major (K, O), O % 4 == 0): thread (4-output chunk c, k-group kg) sums
// its rows with 16-byte weight loads (many loads in flight per thread), then the k-groups are combined in a
// fixed order. scr holds >= 256 * 4 floats.
__device__ void dec_matvec(const float* x, int K, const float* W, const float* b, float* y, int O, float* scr) {
  const int tid = threadIdx.x, nc = O / 4;
  if (nc <= 256) {
    const int G = 256 / nc, kg = tid / nc, c = tid - kg * nc;
    if (kg < G) {
      const int k0 = kg * K / G, k1 = (kg + 1) * K / G;
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
      for (int k = k0; k < k1; ++k) s = s + x[k] * *(const f32x4*)(W + (size_t)k * O + 4 * c);
      *(f32x4*)(scr + (kg * nc + c) * 4) = s;
    }
    __syncthreads();
    if (tid < nc) {
      f32x4 s = *(const f32x4*)(scr + tid * 4);
      for (int g = 1; g < G; ++g) s = s + *(const f32x4*)(scr + (g * nc + tid) * 4);
      if (b) s = s + *(const f32x4*)(b + 4 * tid);
      *(f32x4*)(y + 4 * tid) = s;
    }
    __syncthreads();
  } else {
    for (int c = tid; c < nc; c += 256) {
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 16
      for (int k = 0; k < K; ++k) s = s + x[k] * *(const f32x4*)(W + (size_t)k * O + 4 * c);
      if (b) s = s + *(const f32x4*)(b + 4 * c);
      *(f32x4*)(y + 4 * c) = s;
    }
    __syncthreads();
  }
}

// LayerNorm of a 128-vector in LDS (wave 0 computes the statistics; fixed butterfly order)
__device__ void dec_layernorm(const float* x, const float* gm, const float* bt, float* y, float eps, float* stat) {
  const int tid = threadIdx.x;
  if (tid < 64) {
    const float a0 = x[tid], a1 = x[tid + 64];
    const float mean = warp_sum(a0 + a1) / (float)kDecW;
    const float d0 = a0 - mean, d1 = a1 - mean;
    const float var = warp_sum(d0 * d0 + d1 * d1) / (float)kDecW;
    if (tid == 0) { stat[0] = mean; stat[1] = 1.0f / sqrtf(var + eps); }
  }
  __syncthreads();
  if (tid < kDecW) y[tid] = (x[tid] - stat[0]) * stat[1] * gm[tid] + bt[tid];
  __syncthreads();
}

// Linear maps of a layer composed in fp32 (the decode step then does 3 mat-vecs per layer instead of 7):
//   cw[tap*128 + k][j*32 + n] = sum_m qkvw[tap][k][j*32 + m] * Wj[m][n]   (j = query, key, value)
//   cb[j*32 + n] = sum_m qkvb[j*32 + m] * Wj[m][n] + bj[n]
//   opw[k][n] = sum_m ow[k][m] * pw[m][n],  opb[n] = sum_m ob[m] * pw[m][n] + pb[n]
__global__ __launch_bounds__(256) void prior_decode_prep_kernel(DecArgs a) {
  const DecLayer& ly = a.L[blockIdx.y];
  const int nc = 3 * kDecW * 3 * kDecAW, nb = 3 * kDecAW, no = kDecAW * kDecW;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < nc + nb + no + kDecW; e += gridDim.x * 256) {
    if (e < nc) {
      const int row = e / (3 * kDecAW), col = e - row * (3 * kDecAW), j = col / kDecAW, n = col - j * kDecAW;
      const float* Wj = j == 0 ? ly.qw : j == 1 ? ly.kw : ly.vw;
      float s = 0.f;
      for (int m = 0; m < kDecAW; ++m) s += ly.qkvw[row * 3 * kDecAW + j * kDecAW + m] * Wj[m * kDecAW + n];
      ly.cw[e] = s;
    } else if (e < nc + nb) {
      const int col = e - nc, j = col / kDecAW, n = col - j * kDecAW;
      const float* Wj = j == 0 ? ly.qw : j == 1 ? ly.kw : ly.vw;
      const float* bj = j == 0 ? ly.qb : j == 1 ? ly.kb : ly.vb;
      float s = 0.f;
      for (int m = 0; m < kDecAW; ++m) s += ly.qkvb[j * kDecAW + m] * Wj[m * kDecAW + n];
      ly.cb[col] = s + bj[n];
    } else if (e < nc + nb + no) {
      const int q = e - nc - nb, k = q / kDecW, n = q - k * kDecW;
      float s = 0.f;
      for (int m = 0; m < kDecAW; ++m) s += ly.ow[k * kDecAW + m] * ly.pw[m * kDecW + n];
      ly.opw[q] = s;
    } else {
      const int n = e - nc - nb - no;
      float s = 0.f;
      for (int m = 0; m < kDecAW; ++m) s += ly.ob[m] * ly.pw[m * kDecW + n];
      ly.opb[n] = s + ly.pb[n];
    }
  }
}

// Order-preserving 32-bit key of a float (a larger float has a larger key; -0 < +0, NaNs at the two ends) and
// its inverse.
__device__ __forceinline__ unsigned dec_key(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dec_unkey(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// The k-th largest of v[0 .. n) (1 <= k <= n, n <= 2048, v in LDS), by all 256 threads: a radix select over the
// keys, most significant byte first. Four rounds whatever the data (NaNs and all-equal rows are keys like any
// other): a round counts, in hist[256], the byte of every key that matches the bytes chosen so far; wave 0 then
// finds the byte value d with (#keys with a larger byte) < k <= (#keys with a byte >= d), which becomes the next
// chosen byte, and k drops by the number of keys above it. The invariant 1 <= k <= #matching keys holds from
// round to round, so one d always qualifies; sel is nevertheless preset so that a round can never leave it
// unset. sel holds 2 ints. Ends with every thread holding the result; hist and sel are free again after the
// caller's next barrier.
__device__ float dec_kth_largest(const float* v, int n, int k, int* hist, int* sel) {
  const int tid = threadIdx.x;
  unsigned prefix = 0, mask = 0;
#pragma unroll 1
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[tid] = 0;
    __syncthreads();
    if (tid == 0) { sel[0] = 0; sel[1] = k; }
    for (int e = tid; e < n; e += 256) {
      const unsigned key = dec_key(v[e]);
      if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
    }
    __syncthreads();
    if (tid < 64) {
      // lane L holds the bytes 255 - 4L .. 252 - 4L, largest first; `above` = keys with a larger byte
      int c[4], t = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) { c[j] = hist[255 - 4 * tid - j]; t += c[j]; }
      int above = xl::incl_scan(t) - t;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (above < k && k <= above + c[j]) { sel[0] = 255 - 4 * tid - j; sel[1] = k - above; }
        above += c[j];
      }
    }
    __syncthreads();
    prefix |= (unsigned)sel[0] << shift;
    mask |= 255u << shift;
    k = sel[1];
  }
  return dec_unkey(prefix);
}

// The nucleus (top-p) threshold of the row v[0 .. n) (n <= 2048, v in LDS), by all 256 threads: the logit t* with
// M(> t*) < p Z <= M(>= t*), where M is the mass of the bins of S = {v >= thr} (thr: the top-k threshold, -inf
// without one) beyond a logit value and Z = M(>= -inf). The bins with v >= t* are then exactly the bins of S with
// (mass strictly above their logit) < p Z: the smallest set of top bins whose mass reaches p, ties in or out
// together, the top bin always in.
// Arithmetic: m = max of the row (fmaxf, so NaNs are skipped); a bin of S weighs w = expf((v - m) / temp) in fp32
// (0 <= w <= 1; NaN -> 0), and its mass is the integer q = trunc(w * 2^36): exact for an fp32 w, 0 below 2^-36.
// Masses are summed as 64-bit integers (at most 2048 * 2^36 = 2^47), so every sum is exact and independent of the
// order of the LDS atomics. The target is the integer ceil(p * Zq), formed in fp64 (p and Zq < 2^53 are exact
// there): for an integer mass, M < p Zq <=> M < ceil(p Zq); 1 <= target <= Zq as 0 < p <= 1 <= Zq.
// t* comes from dec_kth_largest's radix select over the keys, most significant byte first, selecting on mass
// instead of count: four rounds whatever the data; a round adds, in hist[256], the mass of every key that matches
// the bytes chosen so far to the bucket of its next byte; wave 0 scans the buckets from the top for the byte d with
// (mass of the larger bytes) < target <= (mass of the bytes >= d), which becomes the next chosen byte, and the
// target drops by the mass above it. 1 <= target <= (matching mass) holds from round to round, so one d always
// qualifies and t* is the key of a bin with a nonzero mass. A row without any mass (m = +-inf or all NaN) leaves
// the target 0: no byte qualifies, the rounds still run, and thr is returned as it came.
// hist holds 256 and sel 2 64-bit words, stat 4 floats; all three are free again after the caller's next barrier.
constexpr float kDecMassScale = 68719476736.f;  // 2^36
__device__ float dec_nucleus_threshold(const float* v, int n, float thr, float temp, float p,
                                       unsigned long long* hist, unsigned long long* sel, float* stat) {
  typedef unsigned long long u64;
  const int tid = threadIdx.x;
  float m = -INFINITY;
  for (int e = tid; e < n; e += 256) m = fmaxf(m, v[e]);
  m = warp_max(m);
  if ((tid & 63) == 0) stat[tid >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(stat[0], stat[1]), fmaxf(stat[2], stat[3]));
  // thread tid owns the bins tid + 256 j: their keys and masses stay in registers over the four rounds
  unsigned key[8];
  u64 q[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int e = tid + 256 * j;
    key[j] = 0;
    q[j] = 0;
    if (e < n) {
      const float lg = v[e];
      key[j] = dec_key(lg);
      if (lg >= thr) {
        float w = expf((lg - m) / temp);
        w = w >= 0.f ? fminf(w, 1.0f) : 0.f;  // NaN: no mass
        q[j] = (u64)(w * kDecMassScale);
      }
    }
  }
  unsigned prefix = 0, mask = 0;
  u64 tgt = 0;
#pragma unroll 1
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[tid] = 0;
    __syncthreads();
    if (tid == 0) { sel[0] = 0; sel[1] = 0; }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (q[j] != 0 && (key[j] & mask) == prefix) atomicAdd(&hist[(key[j] >> shift) & 255u], q[j]);
    __syncthreads();
    if (tid < 64) {
      // lane L holds the bytes 255 - 4L .. 252 - 4L, largest first; `above` = mass of the keys with a larger byte.
      // The 64-bit scan is two int scans of the low 24 and the high bits (t < 2^47: neither can overflow).
      u64 c[4], t = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) { c[j] = hist[255 - 4 * tid - j]; t += c[j]; }
      const int lo = xl::incl_scan((int)(t & 0xFFFFFFu)), hi = xl::incl_scan((int)(t >> 24));
      if (shift == 24) {  // first round: every key matches, lane 63 holds Zq
        const u64 zq = ((u64)(unsigned)__builtin_amdgcn_readlane(hi, 63) << 24) +
                       (u64)(unsigned)__builtin_amdgcn_readlane(lo, 63);
        tgt = (u64)ceil((double)p * (double)zq);
      }
      u64 above = ((u64)(unsigned)hi << 24) + (u64)(unsigned)lo - t;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (above < tgt && tgt <= above + c[j]) { sel[0] = (u64)(255 - 4 * tid - j); sel[1] = tgt - above; }
        above += c[j];
      }
    }
    __syncthreads();
    prefix |= (unsigned)sel[0] << shift;
    mask |= 255u << shift;
    tgt = sel[1];
  }
  if (tgt == 0) return thr;
  return fmaxf(thr, dec_unkey(prefix));
}

// The log-probability of the token written at a step (vqa_prior_decode_scored, include/vqa.h), from the row of
// logits v[0 .. n) in LDS (n = bins: the zero-padded columns n .. ldo are never read):
//   model: (v[tok] - m) - log sum_{e < n} exp(v[e] - m)
//   draw:  (v[tok] - m) / T - log sum_{e: v[e] >= thr} exp((v[e] - m) / T),  -inf when v[tok] < thr
// with m = dec_score_max: the maximum of the row (fmaxf, NaNs skipped). The top bin passes every threshold, so one m
// serves both sums, every exponent is <= 0 and both sums are >= 1. Order: thread tid adds its bins tid, tid + 256, ...
// in index order inside the draw loop; the 256 partial sums are combined by the tree that reduces the draw (slot tid
// += slot tid + w, w = 128 .. 1); no atomics, so a value is bitwise the same from run to run. With T = 1 and thr =
// -inf the division is exact and the two sums add the same numbers in the same order: draw == model bitwise.
// Rounding, against the same fp32 logits and T in exact arithmetic, for |a| <= 32 where a = (v[tok] - m) / T:
//   * a: one fp32 subtraction and one correctly rounded division, <= |a| 2^-23 = 3.8e-6;
//   * a weight w = expf(a_e) is off by at most (|a_e| + 2) 2^-23 relative (its exponent as above, expf <= 2 ulp), so
//     the sum by sum w (|a_e| + 2) 2^-23 / sum w = (E|a_e| + 2) 2^-23 with E over the softmax; E|a_e| = H - log Z
//     <= log n <= log 2048 = 7.6: <= 1.2e-6 in the log;
//   * the additions: at most 8 per thread and 8 tree levels, each 2^-24 relative on positive terms: <= 1e-6;
//   * logf <= 2 ulp of a result <= log 2048: <= 1e-6; the final subtraction rounds a value below 64: <= 1.9e-6.
// In all <= 8.9e-6 (tests/logprob_ref.py: TOL).
__device__ float dec_score_max(const float* v, int n, float* stat) {
  const int tid = threadIdx.x;
  float m = -INFINITY;
  for (int e = tid; e < n; e += 256) m = fmaxf(m, v[e]);
  m = warp_max(m);
  if ((tid & 63) == 0) stat[tid >> 6] = m;
  __syncthreads();
  return fmaxf(fmaxf(stat[0], stat[1]), fmaxf(stat[2], stat[3]));
}
// thread 0, after the tree: lt = the written token's logit (-inf for a token outside the vocabulary)
__device__ __forceinline__ void dec_logprob(const DecArgs& a, size_t at, float lt, float m, float thr, float zmodel,
                                            float zdraw) {
  const float d = lt - m;
  if (a.logp_model) a.logp_model[at] = d - logf(zmodel);
  if (a.logp_draw) a.logp_draw[at] = lt >= thr ? d / a.temp - logf(zdraw) : -INFINITY;
}

template <bool kPrimed, int kFilter>
__global__ __launch_bounds__(256) void prior_decode_kernel(DecArgs a) {
  __shared__ __attribute__((aligned(16))) float x[kDecW], x1[kDecW], hb[kDecW], r1[kDecW];
  __shared__ float ring[kDecMaxLayers][3][kDecW];
  __shared__ __attribute__((aligned(16))) float cat[3 * kDecW], qkv[3 * kDecAW], oh[kDecAW];
  __shared__ float sc[kDecScoreFloats];  // [H][a.scs], see kDecScoreFloats
  __shared__ __attribute__((aligned(16))) float scr[2048];
  __shared__ __attribute__((aligned(16))) float red[32][kDecAW];
  __shared__ float stat[4];
  __shared__ __attribute__((aligned(16))) float bestv[1024];
  __shared__ int besti[256];
  __shared__ int ksel[2];
  const int n = blockIdx.x, tid = threadIdx.x;
  for (int e = tid; e < kDecMaxLayers * 3 * kDecW; e += 256) (&ring[0][0][0])[e] = 0.f;
  int64_t tok = a.start;
  if (tid == 0) a.tokens[(size_t)n * (a.steps + 1)] = a.start;
  __syncthreads();
  for (int i = 0; i < a.steps; ++i) {
    // embedding (autoregressive_fmha.py:119-151)
    if (tid < kDecW) {
      float e = (a.ycond && i == 0) ? a.ycond[(size_t)n * kDecW + tid]
                                    : ((tok >= 0 && tok < a.bins) ? a.emb[(size_t)tok * kDecW + tid] : 0.f);
      e = e * a.emb_scale;
      e = e + a.pos[(size_t)i * kDecW + tid];
      if (a.xcond) e = e + a.xcond[((size_t)n * a.T + i) * kDecW + tid];
      x[tid] = e;
    }
    __syncthreads();
    const int b = i / a.l, p = i - b * a.l;
    for (int L = 0; L < a.depth; ++L) {
      const DecLayer& ly = a.L[L];
      float* aring = &ring[L][0][0];
      dec_layernorm(x, ly.ln1g, ly.ln1b, aring + (i % 3) * kDecW, a.eps, stat);
      // causal conv input [a_{i-2}, a_{i-1}, a_i] (zeros before the sequence start)
      if (tid < kDecW) {
#pragma unroll
        for (int tp = 0; tp < 3; ++tp) {
          const int j = i - 2 + tp;
          cat[tp * kDecW + tid] = j >= 0 ? aring[(j % 3) * kDecW + tid] : 0.f;
        }
      }
      __syncthreads();
      dec_matvec(cat, 3 * kDecW, ly.cw, ly.cb, qkv, 3 * kDecAW, scr);  // [q heads | k heads | v heads]
      const float* qh = qkv;
      const float* kh = qkv + kDecAW;
      const float* vh = qkv + 2 * kDecAW;
      float* kcL = a.kc + (((size_t)n * a.depth + L) * a.T) * kDecAW;
      float* vcL = a.vc + (((size_t)n * a.depth + L) * a.T) * kDecAW;
      if (tid < kDecAW) {
        kcL[(size_t)i * kDecAW + tid] = kh[tid];
        vcL[(size_t)i * kDecAW + tid] = vh[tid];
      }
      __threadfence_block();
      __syncthreads();
      // keys of this position: row: [b*l, i]; col: (b', p) for b' <= b; prev-row: block b-1 (b = 0: value bias)
      int cnt, j0, jstep;
      if (ly.type == 0) { cnt = p + 1; j0 = b * a.l; jstep = 1; }
      else if (ly.type == 1) { cnt = b + 1; j0 = p; jstep = a.l; }
      else { cnt = b > 0 ? a.l : 0; j0 = (b - 1) * a.l; jstep = 1; }
      if (cnt == 0) {
        if (tid < kDecAW) oh[tid] = ly.vb[tid];
        __syncthreads();
      } else {
        const int hd = kDecAW / a.H;
        for (int idx = tid; idx < cnt; idx += 256) {
          const f32x4* kr = (const f32x4*)(kcL + (size_t)(j0 + idx * jstep) * kDecAW);
          const f32x4* qv = (const f32x4*)qh;
          f32x4 kv[kDecAW / 4];
#pragma unroll
          for (int c = 0; c < kDecAW / 4; ++c) kv[c] = kr[c];
          for (int h = 0; h < a.H; ++h) {
            float s = 0.f;
            for (int c = h * hd / 4; c < (h + 1) * hd / 4; ++c) {
              const f32x4 pq = qv[c] * kv[c];
              s += (pq[0] + pq[1]) + (pq[2] + pq[3]);
            }
            sc[h * a.scs + idx] = s * a.scale;
          }
        }
        __syncthreads();
        // per head max and sum (wave h reduces head h)
        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
        if (wave < a.H) {
          float m = -INFINITY;
          float* scw = sc + wave * a.scs;
          for (int idx = lane; idx < cnt; idx += 64) m = fmaxf(m, scw[idx]);
          m = warp_max(m);
          float su = 0.f;
          for (int idx = lane; idx < cnt; idx += 64) {
            const float e = __expf(scw[idx] - m);
            scw[idx] = e;
            su += e;
          }
          su = warp_sum(su);
          if (lane == 0) stat[wave] = 1.0f / su;
        }
        __syncthreads();
        // o[h][d] = sum_j p_j v_j[h][d]: thread (4-channel chunk c4 = tid & 7, key slice sl = tid >> 3) over keys
        // sl, sl + 32, ... with 16-byte loads; slices combined in a fixed order
        {
          const int c4 = tid & 7, sl = tid >> 3, h = 4 * c4 / hd;
          const float* sch = sc + h * a.scs;
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
          for (int idx = sl; idx < cnt; idx += 32)
            acc = acc + sch[idx] * *(const f32x4*)(vcL + (size_t)(j0 + idx * jstep) * kDecAW + 4 * c4);
          *(f32x4*)(&red[sl][4 * c4]) = acc;
        }
        __syncthreads();
        if (tid < kDecAW) {
          float o = red[0][tid];
          for (int sl = 1; sl < 32; ++sl) o += red[sl][tid];
          oh[tid] = o * stat[tid / hd];
        }
        __syncthreads();
      }
      dec_matvec(oh, kDecAW, ly.opw, ly.opb, r1, kDecW, scr);  // output EinsumDense o proj
      if (tid < kDecW) x1[tid] = x[tid] + r1[tid];
      __syncthreads();
      dec_layernorm(x1, ly.ln2g, ly.ln2b, hb, a.eps, stat);
      dec_matvec(hb, kDecW, ly.mw, ly.mb, cat, kDecW, scr);  // res2 (cat reused)
      if (tid < kDecW) x[tid] = cat[tid] + x1[tid];
      __syncthreads();
    }
    // a primed step: the next input is the prime's; its head runs only for the logits output
    bool primed = false;
    if constexpr (kPrimed) {
      primed = i < a.prime_len;
      if (primed && !a.logits) {
        tok = a.prime[(size_t)n * a.prime_len + i];
        if (tid == 0) a.tokens[(size_t)n * (a.steps + 1) + i + 1] = tok;
        if constexpr (kFilter >= 2) {
          if (a.kept && tid == 0) a.kept[(size_t)n * a.steps + i] = 0;
        }
        if constexpr (kFilter == 3) {
          if (a.logp_model && tid == 0) a.logp_model[(size_t)n * a.steps + i] = 0.f;
          if (a.logp_draw && tid == 0) a.logp_draw[(size_t)n * a.steps + i] = 0.f;
        }
        continue;
      }
    }
    // output head + Gumbel-max
    dec_matvec(x, kDecW, a.hw, a.hb, scr, a.ldo, bestv);  // scr holds the logits (ldo >= bins columns)
    float thr = -INFINITY;  // top-k: only the bins with logit >= the k-th largest of the row take part
    if constexpr (kFilter != 0) {
      if (a.topk > 0) thr = dec_kth_largest(scr, a.bins, a.topk, besti, ksel);
    }
    if constexpr (kFilter >= 2) {
      // bestv (the head mat-vec's scratch) is free: 256 + 2 64-bit words of it hold the mass histogram
      if (a.topp < 1.0f)
        thr = dec_nucleus_threshold(scr, a.bins, thr, a.temp, a.topp, (unsigned long long*)bestv,
                                    (unsigned long long*)bestv + 256, stat);
    }
    float smax = 0.f, zm = 0.f, zd = 0.f;  // kFilter = 3: the row maximum, this thread's share of the two sums
    if constexpr (kFilter == 3) smax = dec_score_max(scr, a.bins, stat);
    float bv = -INFINITY;
    int bi = 0, nk = 0;  // nk: this thread's bins that take part (kFilter >= 2)
    for (int v = tid; v < a.bins; v += 256) {
      const float lg = scr[v];
      if (a.logits) a.logits[((size_t)n * a.steps + i) * a.bins + v] = lg;
      if constexpr (kFilter == 3) zm += expf(lg - smax);
      if constexpr (kFilter != 0) {
        if (!(lg >= thr)) continue;
      }
      if constexpr (kFilter >= 2) ++nk;
      if constexpr (kFilter == 3) zd += expf((lg - smax) / a.temp);
      const float u = prior_uniform(a.seed, (uint64_t)n, (uint64_t)i, (uint64_t)v);
      float z;
      if constexpr (kFilter != 0) z = lg / a.temp + (-logf(-logf(u)));
      else z = lg + (-logf(-logf(u)));
      if (z > bv) { bv = z; bi = v; }
    }
    __syncthreads();
    bestv[tid] = bv;
    besti[tid] = bi;
    // kFilter = 2: the logits are dead past the barrier above and the counts ride the tree in scr. kFilter = 3 still
    // needs the written token's logit after the tree: the counts and the two sums ride in red (the attention's
    // scratch, 1024 floats, idle from a layer's last barrier to the next step) and scr stays whole.
    int* nkept = kFilter == 3 ? (int*)&red[0][0] : (int*)scr;
    float* zsum = &red[0][0] + 256;  // [256] model, [256] draw
    if constexpr (kFilter >= 2) nkept[tid] = nk;
    if constexpr (kFilter == 3) { zsum[tid] = zm; zsum[256 + tid] = zd; }
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (tid < w) {
        const float ov = bestv[tid + w];
        const int oi = besti[tid + w];
        if (ov > bestv[tid] || (ov == bestv[tid] && oi < besti[tid])) { bestv[tid] = ov; besti[tid] = oi; }
        if constexpr (kFilter >= 2) nkept[tid] += nkept[tid + w];
        if constexpr (kFilter == 3) { zsum[tid] += zsum[tid + w]; zsum[256 + tid] += zsum[256 + tid + w]; }
      }
      __syncthreads();
    }
    if constexpr (kFilter >= 2) {
      if (a.kept && tid == 0) a.kept[(size_t)n * a.steps + i] = nkept[0];
    }
    int64_t samp = besti[0];
    if constexpr (kPrimed) {
      if (primed) samp = a.prime[(size_t)n * a.prime_len + i];
    }
    if constexpr (kFilter == 3) {
      if (tid == 0)
        dec_logprob(a, (size_t)n * a.steps + i, (samp >= 0 && samp < a.bins) ? scr[samp] : -INFINITY, smax, thr,
                    zsum[0], zsum[256]);
    }
    if (tid == 0) a.tokens[(size_t)n * (a.steps + 1) + i + 1] = samp;
    tok = a.forced ? a.forced[(size_t)n * (a.steps + 1) + i + 1] : samp;
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------
constexpr size_t kDecComposed = (size_t)3 * kDecW * 3 * kDecAW + 3 * kDecAW + kDecAW * kDecW + kDecW;  // floats/layer

}  // namespace vqa

using namespace vqa;

extern "C" size_t vqa_prior_decode_cache_bytes(int N, int depth, int ctx) {
  if (N < 1 || depth < 1 || ctx < 1) return 0;
  return ((size_t)2 * N * depth * ctx * kDecAW + (size_t)depth * kDecComposed) * sizeof(float);
}

extern "C" int vqa_prior_decode_scored(const vqa_prior_layer* layers, int depth, const float* x_embedding,
                                       const float* pos_embedding, const float* out_kernel, const float* out_bias,
                                       const float* ycond, const float* xcond, const int64_t* forced, float* logits,
                                       int64_t* tokens, void* cache, size_t cache_bytes, int N, int steps, int ctx,
                                       int width, int heads, int blocks, int bins, int out_ld, int64_t start,
                                       uint64_t seed, const int64_t* prime, int prime_len, float temperature,
                                       int top_k, float top_p, int32_t* kept, float* logp_model, float* logp_draw,
                                       vqa_stream_t stream) {
  VQA_ARG(layers && x_embedding && pos_embedding && out_kernel && out_bias && tokens && cache && N > 0 && steps > 0 &&
              steps <= ctx && blocks > 0 && ctx % blocks == 0 && bins > 0 && out_ld >= bins && out_ld % 4 == 0 &&
              out_ld <= 2048,
          "prior_decode: bad arguments (bins %d, out_ld %d)", bins, out_ld);
  // the prime, the temperature and top-k are settled here, before anything is launched
  VQA_ARG(prime_len >= 0 && prime_len <= steps, "prior_decode: prime_len %d outside [0, steps %d]", prime_len, steps);
  VQA_ARG(prime || prime_len == 0, "prior_decode: prime_len %d without a prime", prime_len);
  VQA_ARG(!(prime && forced), "prior_decode: a prime and forced tokens are mutually exclusive");
  VQA_ARG(std::isfinite(temperature) && temperature > 0.f, "prior_decode: temperature %g is not finite and > 0",
          (double)temperature);
  VQA_ARG(top_k >= 0 && top_k <= bins, "prior_decode: top_k %d outside [0, bins %d]", top_k, bins);
  VQA_ARG(std::isfinite(top_p) && top_p > 0.f && top_p <= 1.0f, "prior_decode: top_p %g is not finite and in (0, 1]",
          (double)top_p);
  VQA_REQUIRE(depth > 0 && depth <= kDecMaxLayers && width == kDecW && heads > 0 && kDecAW % heads == 0 &&
                  kDecAW / heads <= 32 && ctx / blocks <= kDecMaxL && heads <= 4,
              VQA_E_UNSUPPORTED, "prior_decode: depth %d width %d heads %d block %d unsupported", depth, width, heads,
              ctx / blocks);
  // the score scratch holds `heads` rows of max(block length, blocks) floats (kDecScoreFloats, above)
  const int scs = ctx / blocks > blocks ? ctx / blocks : blocks;
  VQA_REQUIRE((long long)heads * scs <= kDecScoreFloats, VQA_E_UNSUPPORTED,
              "prior_decode: heads %d x max(block length %d, blocks %d) exceeds the %d-float score scratch", heads,
              ctx / blocks, blocks, kDecScoreFloats);
  VQA_ARG(cache_bytes >= vqa_prior_decode_cache_bytes(N, depth, ctx), "prior_decode: cache too small");
  DecArgs a;
  float* comp = (float*)cache + (size_t)2 * N * depth * ctx * kDecAW;
  for (int L = 0; L < depth; ++L) {
    const vqa_prior_layer& s = layers[L];
    VQA_ARG(s.attn_type >= 0 && s.attn_type <= 2, "prior_decode: layer %d attention type %d", L, s.attn_type);
    float* c = comp + (size_t)L * kDecComposed;
    a.L[L] = DecLayer{s.ln1_gamma, s.ln1_beta, s.qkv_kernel, s.qkv_bias, s.query_kernel, s.query_bias, s.key_kernel,
                      s.key_bias, s.value_kernel, s.value_bias, s.out_kernel, s.out_bias, s.proj_kernel, s.proj_bias,
                      s.ln2_gamma, s.ln2_beta, s.mlp_kernel, s.mlp_bias, s.attn_type,
                      c, c + 3 * kDecW * 3 * kDecAW, c + 3 * kDecW * 3 * kDecAW + 3 * kDecAW,
                      c + 3 * kDecW * 3 * kDecAW + 3 * kDecAW + kDecAW * kDecW};
  }
  a.emb = x_embedding; a.pos = pos_embedding; a.hw = out_kernel; a.hb = out_bias;
  a.ycond = ycond; a.xcond = xcond; a.forced = forced; a.logits = logits; a.tokens = tokens;
  a.kc = (float*)cache;
  a.vc = (float*)cache + (size_t)N * depth * ctx * kDecAW;
  a.N = N; a.steps = steps; a.T = ctx; a.depth = depth; a.H = heads; a.l = ctx / blocks; a.bins = bins; a.ldo = out_ld;
  a.scs = scs;
  a.start = start; a.seed = seed;
  a.scale = 1.0f / sqrtf((float)(kDecAW / heads));
  a.emb_scale = sqrtf((float)width);
  a.eps = 1e-6f;
  a.prime = prime_len > 0 ? prime : nullptr;
  a.prime_len = prime_len;
  a.topk = (top_k > 0 && top_k < bins) ? top_k : 0;  // 0 and bins: every bin takes part
  a.temp = temperature;
  a.topp = top_p;
  a.kept = kept;
  a.logp_model = logp_model;
  a.logp_draw = logp_draw;
  // 0: the unfiltered decode; 1: a temperature and / or top-k; 2: top-p on (top_p = 1 is off, decided here: the
  // filter is not run, so weights that underflow drop no bin) or the kept counts asked for; 3: a log-probability
  // output asked for (2 plus the two log-sums; temperature 1 divides exactly and draws the unfiltered decode's tokens)
  const int filter = (logp_model || logp_draw) ? 3
                     : (top_p < 1.0f || kept)  ? 2
                     : (a.topk > 0 || temperature != 1.0f) ? 1 : 0;
  hipLaunchKernelGGL(prior_decode_prep_kernel, dim3(64, depth), dim3(256), 0, (hipStream_t)stream, a);
  VQA_LAUNCHED("prior_decode_prep_kernel");
  const bool primed = prime_len > 0;
  void (*kern)(DecArgs) =
      primed ? (filter == 3   ? prior_decode_kernel<true, 3>
                : filter == 2 ? prior_decode_kernel<true, 2>
                : filter      ? prior_decode_kernel<true, 1>
                              : prior_decode_kernel<true, 0>)
             : (filter == 3   ? prior_decode_kernel<false, 3>
                : filter == 2 ? prior_decode_kernel<false, 2>
                : filter      ? prior_decode_kernel<false, 1>
                              : prior_decode_kernel<false, 0>);
  hipLaunchKernelGGL(kern, dim3(N), dim3(256), 0, (hipStream_t)stream, a);
  VQA_LAUNCHED("prior_decode_kernel");
  return VQA_OK;
}

extern "C" int vqa_prior_decode_filtered(const vqa_prior_layer* layers, int depth, const float* x_embedding,
                                         const float* pos_embedding, const float* out_kernel, const float* out_bias,
                                         const float* ycond, const float* xcond, const int64_t* forced, float* logits,
                                         int64_t* tokens, void* cache, size_t cache_bytes, int N, int steps, int ctx,
                                         int width, int heads, int blocks, int bins, int out_ld, int64_t start,
                                         uint64_t seed, const int64_t* prime, int prime_len, float temperature,
                                         int top_k, float top_p, int32_t* kept, vqa_stream_t stream) {
  return vqa_prior_decode_scored(layers, depth, x_embedding, pos_embedding, out_kernel, out_bias, ycond, xcond, forced,
                                 logits, tokens, cache, cache_bytes, N, steps, ctx, width, heads, blocks, bins, out_ld,
                                 start, seed, prime, prime_len, temperature, top_k, top_p, kept, nullptr, nullptr,
                                 stream);
}

extern "C" int vqa_prior_decode_primed(const vqa_prior_layer* layers, int depth, const float* x_embedding,
                                       const float* pos_embedding, const float* out_kernel, const float* out_bias,
                                       const float* ycond, const float* xcond, const int64_t* forced, float* logits,
                                       int64_t* tokens, void* cache, size_t cache_bytes, int N, int steps, int ctx,
                                       int width, int heads, int blocks, int bins, int out_ld, int64_t start,
                                       uint64_t seed, const int64_t* prime, int prime_len, float temperature,
                                       int top_k, vqa_stream_t stream) {
  return vqa_prior_decode_filtered(layers, depth, x_embedding, pos_embedding, out_kernel, out_bias, ycond, xcond, forced,
                                   logits, tokens, cache, cache_bytes, N, steps, ctx, width, heads, blocks, bins, out_ld,
                                   start, seed, prime, prime_len, temperature, top_k, 1.0f, nullptr, stream);
}

extern "C" int vqa_prior_decode(const vqa_prior_layer* layers, int depth, const float* x_embedding,
                                const float* pos_embedding, const float* out_kernel, const float* out_bias,
                                const float* ycond, const float* xcond, const int64_t* forced, float* logits,
                                int64_t* tokens, void* cache, size_t cache_bytes, int N, int steps, int ctx, int width,
                                int heads, int blocks, int bins, int out_ld, int64_t start, uint64_t seed,
                                vqa_stream_t stream) {
  return vqa_prior_decode_primed(layers, depth, x_embedding, pos_embedding, out_kernel, out_bias, ycond, xcond, forced,
                                 logits, tokens, cache, cache_bytes, N, steps, ctx, width, heads, blocks, bins, out_ld,
                                 start, seed, nullptr, 0, 1.0f, 0, stream);
}
