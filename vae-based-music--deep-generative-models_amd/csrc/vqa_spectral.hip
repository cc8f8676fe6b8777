// vqa_spectral.hip — multi-resolution spectral loss and its gradient (gfx950).
//
// Replaces the reference's per-level
//   data_utils.py:25-30  spectral(x) = |tf.signal.stft(x, frame_length=win, frame_step=hop, fft_length=n_fft)|
//   data_utils.py:33-40  norm(x)     = tf.norm(x, 'fro', axis=[-2, -1])
//   vqvae.py:309-326     _multispectral_loss = mean_b mean_res norm(S_x - S_r) / norm(S_x)
// and the GradientTape backward of that expression w.r.t. the reconstruction (vqvae.py:143).
//
// One wave transforms a PAIR of windowed STFT frames by one complex fp32 FFT, persistent over the pairs (the pair
// kernels: vqa_spectral_stockham.hip, vqa_spectral_fourstep.hip; twiddles and window evaluated once per call in fp64
// by spec_tables_kernel). The target's magnitudes |X_k| are written once per step; against them the
// per-bin magnitudes |R_k| give the frame's partial sums sum (|X|-|R|)^2 and sum |X|^2, and — for the
// gradient — the bin gradient G_k = (|R_k| - |X_k|) R_k / |R_k| (0 where |R_k| = 0, TF's abs'(0)) is mapped
// back to the time domain by the adjoint of the one-sided rfft (an inverse FFT of the Hermitian extension
// of G), windowed, and written unscaled per frame. The per-item scale 1 / (nres * B * ||S_x - S_r|| *
// ||S_x||) is known only after every frame of the item is done, so a second kernel reduces the partial sums
// per (item, resolution) and a third overlap-adds the frame gradients (fixed summation order:
// deterministic) and applies the scales. No atomics, no host sync, graph-capturable.
// This unit: the table, scale and overlap-add kernels, the workspace layout, the choice of engine per n_fft
// (dispatch_pairs) and the C entries.
#include "vqa_spectral.h"

namespace vqa {

// the tables of every resolution (N twiddles, win window values each: spec_twiddle / spec_hann)
struct SpecTables {
  float* tw[SPEC_MAX_RES];
  float* wn[SPEC_MAX_RES];
  int N[SPEC_MAX_RES], win[SPEC_MAX_RES];
  int nres;
};

__global__ __launch_bounds__(256) void spec_tables_kernel(SpecTables t) {
  const int res = blockIdx.y;
  const int N = t.N[res], W = t.win[res];
  for (int k = blockIdx.x * 256 + threadIdx.x; k < N; k += gridDim.x * 256) ((f32x2*)t.tw[res])[k] = spec_twiddle(k, N);
  for (int n = blockIdx.x * 256 + threadIdx.x; n < W; n += gridDim.x * 256) t.wn[res][n] = spec_hann(n, W);
}

struct SpecScaleArgs {
  const float* part[SPEC_MAX_RES];
  int F[SPEC_MAX_RES];
  float* lossbr;  // (B, nres) per item and resolution: ||S_x - S_r|| / ||S_x||
  float* scale;   // (B, nres): inv / (||S_x - S_r|| * ||S_x||)
  int nres;
  float inv;  // 1 / (nres * B)
};

__global__ __launch_bounds__(256) void spec_scale_kernel(SpecScaleArgs a) {
  __shared__ float red[4];
  const int b = blockIdx.x / a.nres, res = blockIdx.x - b * a.nres;
  const int F = a.F[res];
  const float* p = a.part[res] + (size_t)b * F * 2;
  float sd = 0.f, sx = 0.f;
  for (int f = threadIdx.x; f < F; f += 256) {
    sd += p[2 * f];
    sx += p[2 * f + 1];
  }
  sd = block_sum_256(sd, red);
  __syncthreads();
  sx = block_sum_256(sx, red);
  if (threadIdx.x == 0) {
    const float nd = sqrtf(sd), nx = sqrtf(sx);
    a.lossbr[blockIdx.x] = nd / nx;
    a.scale[blockIdx.x] = a.inv / (nd * nx);
  }
}

struct SpecGatherArgs {
  const float* fg[SPEC_MAX_RES];
  int F[SPEC_MAX_RES], hop[SPEC_MAX_RES], win[SPEC_MAX_RES];
  const float* lossbr;
  const float* scale;
  float* dr;         // (B, T) or null (loss only)
  float* loss_out;   // [1]: mean_b mean_res lossbr
  float* item_loss;  // (B) or null: mean_res lossbr
  int B, T, nres;
};

__global__ __launch_bounds__(256) void spec_gather_kernel(SpecGatherArgs a) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float tot = 0.f;
    for (int b = 0; b < a.B; ++b) {
      float s = 0.f;
      for (int r = 0; r < a.nres; ++r) s += a.lossbr[b * a.nres + r];
      s = s / (float)a.nres;
      if (a.item_loss) a.item_loss[b] = s;
      tot += s;
    }
    a.loss_out[0] = tot / (float)a.B;
  }
  if (!a.dr) return;
  const long long n = (long long)a.B * a.T;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int b = (int)(i / a.T), t = (int)(i - (long long)b * a.T);
    float acc = 0.f;
    for (int r = 0; r < a.nres; ++r) {
      const int hop = a.hop[r], win = a.win[r], F = a.F[r];
      const int f_hi = min(F - 1, t / hop);
      const int f_lo = t >= win ? (t - win) / hop + 1 : 0;
      const float* g = a.fg[r] + (size_t)b * F * win;
      float s = 0.f;
      for (int f = f_lo; f <= f_hi; ++f) s += g[(size_t)f * win + (t - f * hop)];
      acc += a.scale[b * a.nres + r] * s;
    }
    a.dr[i] = acc;
  }
}

// The same overlap-add for the usual shapes (<= 4 resolutions, <= 8 frames over a sample, T < 2^24): item =
// blockIdx.y (no 64-bit division per sample), and every frame read of every resolution is issued before the
// sums (clamped addresses; a frame past the sample's range is loaded and not added), so a thread's 15-odd
// loads are in flight together instead of one trip-count-dependent loop iteration at a time. Same sums in the
// same order: bit-identical to spec_gather_kernel.
constexpr int kGatherMaxRes = 4, kGatherMaxF = 8;
__global__ __launch_bounds__(256) void spec_gather8_kernel(SpecGatherArgs a) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    float tot = 0.f;
    for (int b = 0; b < a.B; ++b) {
      float s = 0.f;
      for (int r = 0; r < a.nres; ++r) s += a.lossbr[b * a.nres + r];
      s = s / (float)a.nres;
      if (a.item_loss) a.item_loss[b] = s;
      tot += s;
    }
    a.loss_out[0] = tot / (float)a.B;
  }
  const int b = blockIdx.y;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < a.T; t += gridDim.x * 256) {
    float v[kGatherMaxRes][kGatherMaxF];
    int nf[kGatherMaxRes];
#pragma unroll
    for (int r = 0; r < kGatherMaxRes; ++r) {
      if (r >= a.nres) break;  // uniform
      const int hop = a.hop[r], win = a.win[r], F = a.F[r];
      const int f_hi = min(F - 1, t / hop);
      const int f_lo = t >= win ? (t - win) / hop + 1 : 0;
      nf[r] = f_hi - f_lo + 1;
      const float* g = a.fg[r] + (size_t)b * F * win;
#pragma unroll
      for (int j = 0; j < kGatherMaxF; ++j) {
        const int f = min(f_lo + j, f_hi);
        v[r][j] = g[(size_t)f * win + min(t - f * hop, win - 1)];
      }
    }
    float acc = 0.f;
#pragma unroll
    for (int r = 0; r < kGatherMaxRes; ++r) {
      if (r >= a.nres) break;
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < kGatherMaxF; ++j)
        if (j < nf[r]) s += v[r][j];
      acc += a.scale[b * a.nres + r] * s;
    }
    a.dr[(size_t)b * a.T + t] = acc;
  }
}

static bool spec_gather8_ok(const SpecGatherArgs& a) {
  if (!a.dr || a.nres > kGatherMaxRes || a.T >= (1 << 24) || a.B > 65535) return false;  // items = grid rows
  for (int r = 0; r < a.nres; ++r)
    if ((a.win[r] + a.hop[r] - 1) / a.hop[r] > kGatherMaxF) return false;
  return true;
}

static bool spec_n_ok(int n) { return n == 256 || n == 512 || n == 1024 || n == 2048; }

template <int MODE>
static int dispatch_pairs(int n_fft, const SpecPairArgs& pa, hipStream_t s) {
  switch (n_fft) {
    // the four-step form where it is faster (2048: 8 waves, two per SIMD, 84 -> 58 us per gradient launch at config 2);
    // the Stockham form (one radix-8 / 16 / 4 pass per LDS round trip) keeps fewer VALU instructions per pair for
    // the shorter transforms, which run at several waves per SIMD either way (round 6, profiles/r6_spectral.txt)
    case 256:
    case 512:
    case 1024: return spec_pairs_stockham(MODE, n_fft, pa, s);
    case 2048: return spec_pairs_fourstep(MODE, n_fft, pa, s);
    default: set_error("spectral: n_fft %d unsupported (256, 512, 1024, 2048)", n_fft); return VQA_E_UNSUPPORTED;
  }
}

static size_t align64(size_t n) { return (n + 63) & ~(size_t)63; }

// Target region (floats; per resolution: twiddles 2N | window | |S_x| (B*F, N/2+1)) and loss workspace
// (per resolution: frame gradients (grad only) | per-frame partials; then per-item losses | scales).
struct SpecLayout {
  size_t tw[SPEC_MAX_RES], wn[SPEC_MAX_RES], tm[SPEC_MAX_RES], target;
  size_t fg[SPEC_MAX_RES], part[SPEC_MAX_RES], tail, loss;
  int F[SPEC_MAX_RES];
};

static int spec_layout(int B, int T, const int* n_fft, const int* hop, const int* win, int nres, bool grad,
                       SpecLayout* L) {
  if (B <= 0 || T <= 0 || nres <= 0 || nres > SPEC_MAX_RES || !n_fft || !hop || !win) return VQA_E_INVALID_ARG;
  size_t o = 0;
  for (int r = 0; r < nres; ++r) {
    if (hop[r] <= 0 || win[r] <= 0 || win[r] > n_fft[r] || win[r] > T || !spec_n_ok(n_fft[r])) return VQA_E_INVALID_ARG;
    L->F[r] = 1 + (T - win[r]) / hop[r];
    L->tw[r] = o;
    o += align64((size_t)2 * n_fft[r]);
    L->wn[r] = o;
    o += align64((size_t)win[r]);
    L->tm[r] = o;
    o += align64((size_t)B * L->F[r] * (n_fft[r] / 2 + 1));
  }
  L->target = o * sizeof(float);
  o = 0;
  for (int r = 0; r < nres; ++r) {
    L->fg[r] = o;
    if (grad) o += align64((size_t)B * L->F[r] * win[r]);
    L->part[r] = o;
    o += align64((size_t)B * L->F[r] * 2);
  }
  L->tail = o;
  o += align64((size_t)B * nres * 2);
  L->loss = o * sizeof(float);
  return VQA_OK;
}

static int spec_target(const float* x, float* tg, const SpecLayout& L, int B, int T, const int* n_fft, const int* hop,
                       const int* win, int nres, hipStream_t s) {
  SpecTables tb{};
  int maxn = 0;
  for (int i = 0; i < nres; ++i) {
    tb.tw[i] = tg + L.tw[i];
    tb.wn[i] = tg + L.wn[i];
    tb.N[i] = n_fft[i];
    tb.win[i] = win[i];
    maxn = n_fft[i] > maxn ? n_fft[i] : maxn;
  }
  tb.nres = nres;
  hipLaunchKernelGGL(spec_tables_kernel, dim3((maxn + 255) / 256, nres), dim3(256), 0, s, tb);
  VQA_LAUNCHED("spec_tables_kernel");
  for (int i = 0; i < nres; ++i) {
    SpecPairArgs pa{x, nullptr, tg + L.tm[i], nullptr, tg + L.tw[i], tg + L.wn[i], B, T, L.F[i], hop[i], win[i]};
    if (int rc = dispatch_pairs<PAIR_MAG>(n_fft[i], pa, s)) return rc;
  }
  return VQA_OK;
}

static int spec_loss(const float* tg, const float* r, float* loss_out, float* dr, float* item_loss, float* ws,
                     const SpecLayout& L, int B, int T, const int* n_fft, const int* hop, const int* win, int nres,
                     hipStream_t s) {
  const bool grad = dr != nullptr;
  SpecScaleArgs sa{};
  SpecGatherArgs ga{};
  for (int i = 0; i < nres; ++i) {
    SpecPairArgs pa{r, tg + L.tm[i], ws + L.fg[i], ws + L.part[i], tg + L.tw[i], tg + L.wn[i], B, T, L.F[i], hop[i],
                    win[i]};
    const int rc = grad ? dispatch_pairs<PAIR_GRAD>(n_fft[i], pa, s) : dispatch_pairs<PAIR_LOSS>(n_fft[i], pa, s);
    if (rc != VQA_OK) return rc;
    sa.part[i] = ws + L.part[i];
    sa.F[i] = L.F[i];
    ga.fg[i] = ws + L.fg[i];
    ga.F[i] = L.F[i];
    ga.hop[i] = hop[i];
    ga.win[i] = win[i];
  }
  sa.lossbr = ws + L.tail;
  sa.scale = ws + L.tail + (size_t)B * nres;
  sa.nres = nres;
  sa.inv = (float)(1.0 / ((double)nres * (double)B));
  hipLaunchKernelGGL(spec_scale_kernel, dim3(B * nres), dim3(256), 0, s, sa);
  VQA_LAUNCHED("spec_scale_kernel");
  ga.lossbr = sa.lossbr;
  ga.scale = sa.scale;
  ga.dr = dr;
  ga.loss_out = loss_out;
  ga.item_loss = item_loss;
  ga.B = B;
  ga.T = T;
  ga.nres = nres;
  if (spec_gather8_ok(ga)) {
    int nx = (T + 255) / 256;
    if (nx > 1024) nx = 1024;
    hipLaunchKernelGGL(spec_gather8_kernel, dim3(nx, B), dim3(256), 0, s, ga);
    VQA_LAUNCHED("spec_gather8_kernel");
    return VQA_OK;
  }
  long long nb = grad ? ((long long)B * T + 255) / 256 : 1;
  if (nb > 8192) nb = 8192;
  hipLaunchKernelGGL(spec_gather_kernel, dim3((int)nb), dim3(256), 0, s, ga);
  VQA_LAUNCHED("spec_gather_kernel");
  return VQA_OK;
}

}  // namespace vqa

using namespace vqa;

#define SPEC_SHAPE_ERR "spectral: bad shape (B=%d T=%d nres=%d; need 0 < win <= n_fft, win <= T, hop > 0, " \
                       "n_fft in {256, 512, 1024, 2048})"

extern "C" size_t vqa_spectral_target_workspace(int B, int T, const int* n_fft, const int* hop, const int* win,
                                                int nres) {
  SpecLayout L;
  return spec_layout(B, T, n_fft, hop, win, nres, false, &L) == VQA_OK ? L.target : 0;
}

extern "C" int vqa_spectral_target(const float* x, void* target, size_t target_bytes, int B, int T, const int* n_fft,
                                   const int* hop, const int* win, int nres, vqa_stream_t stream) {
  VQA_ARG(x && target, "spectral_target: null pointer");
  SpecLayout L;
  VQA_ARG(spec_layout(B, T, n_fft, hop, win, nres, false, &L) == VQA_OK, SPEC_SHAPE_ERR, B, T, nres);
  VQA_ARG(target_bytes >= L.target, "spectral_target: buffer %zu < %zu bytes", target_bytes, L.target);
  return spec_target(x, (float*)target, L, B, T, n_fft, hop, win, nres, (hipStream_t)stream);
}

extern "C" size_t vqa_spectral_loss_target_workspace(int B, int T, const int* n_fft, const int* hop, const int* win,
                                                     int nres, int with_grad) {
  SpecLayout L;
  return spec_layout(B, T, n_fft, hop, win, nres, with_grad != 0, &L) == VQA_OK ? L.loss : 0;
}

extern "C" int vqa_spectral_loss_target(const void* target, const float* r, float* loss_out, float* dr,
                                        float* item_loss, int B, int T, const int* n_fft, const int* hop,
                                        const int* win, int nres, void* workspace, size_t ws_bytes,
                                        vqa_stream_t stream) {
  VQA_ARG(target && r && loss_out, "spectral_loss_target: null pointer");
  SpecLayout L;
  VQA_ARG(spec_layout(B, T, n_fft, hop, win, nres, dr != nullptr, &L) == VQA_OK, SPEC_SHAPE_ERR, B, T, nres);
  VQA_ARG(workspace && ws_bytes >= L.loss, "spectral_loss_target: workspace %zu < %zu bytes", ws_bytes, L.loss);
  return spec_loss((const float*)target, r, loss_out, dr, item_loss, (float*)workspace, L, B, T, n_fft, hop, win, nres,
                   (hipStream_t)stream);
}

extern "C" size_t vqa_spectral_loss_workspace(int B, int T, const int* n_fft, const int* hop, const int* win,
                                              int nres, int with_grad) {
  SpecLayout L;
  if (spec_layout(B, T, n_fft, hop, win, nres, with_grad != 0, &L) != VQA_OK) return 0;
  return L.target + L.loss;
}

extern "C" int vqa_spectral_loss(const float* x, const float* r, float* loss_out, float* dr, float* item_loss, int B,
                                 int T, const int* n_fft, const int* hop, const int* win, int nres, void* workspace,
                                 size_t ws_bytes, vqa_stream_t stream) {
  VQA_ARG(x && r && loss_out, "spectral_loss: null pointer");
  SpecLayout L;
  VQA_ARG(spec_layout(B, T, n_fft, hop, win, nres, dr != nullptr, &L) == VQA_OK, SPEC_SHAPE_ERR, B, T, nres);
  VQA_ARG(workspace && ws_bytes >= L.target + L.loss, "spectral_loss: workspace %zu < %zu bytes", ws_bytes,
          L.target + L.loss);
  hipStream_t s = (hipStream_t)stream;
  float* tg = (float*)workspace;
  if (int rc = spec_target(x, tg, L, B, T, n_fft, hop, win, nres, s)) return rc;
  return spec_loss(tg, r, loss_out, dr, item_loss, tg + L.target / sizeof(float), L, B, T, n_fft, hop, win, nres, s);
}

extern "C" int vqa_stft_magnitude(const float* x, float* mag, int B, int T, int n_fft, int hop, int win,
                                  vqa_stream_t stream) {
  VQA_ARG(x && mag && B > 0 && hop > 0 && win > 0 && win <= n_fft && win <= T,
          "stft_magnitude: bad arguments (B=%d T=%d n_fft=%d hop=%d win=%d)", B, T, n_fft, hop, win);
  const int F = 1 + (T - win) / hop;
  // no workspace in this entry point: the pair kernels evaluate their twiddles and window themselves
  SpecPairArgs pa{x, nullptr, mag, nullptr, nullptr, nullptr, B, T, F, hop, win};
  return dispatch_pairs<PAIR_MAG_SELF>(n_fft, pa, (hipStream_t)stream);
}
