// vqa_runtime.hip — error reporting, launch support, the MSE loss, the step's metric trackers and the synthetic
// batch (gfx950).
//
//   vqa_mse_loss     : keras MeanSquaredError(reduction=NONE) + tf.reduce_mean (vqvae.py:91,125) fused with
//                      its gradient and the spectral-loss gradient add.
//   vqa_step_metrics : the step's metric trackers as one launch; vqa_step_metrics_if leaves them as they are
//                      when the step was skipped (a device flag, so a captured step replays the decision).
//   vqa_synthetic_batch : the on-device synthetic waveform feed.
#include "vqa_launch.h"
#include <stdarg.h>
#include <stdio.h>
#include <algorithm>
#include <map>
#include <mutex>
#include <utility>

namespace vqa {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ---- launch support (vqa_launch.h)
int cu_count() {
  static const int n = [] {
    int dev = 0, v = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) {
      (void)hipGetLastError();
      v = 256;
    }
    return v;
  }();
  return n;
}

static std::mutex g_launch_mu;  // guards the two stores below

int raise_dyn_lds(const void* fn, size_t bytes, const char* what) {
  if (bytes <= 65536) return VQA_OK;
  static std::map<const void*, size_t> raised;
  std::lock_guard<std::mutex> lock(g_launch_mu);
  size_t& have = raised[fn];
  if (bytes <= have) return VQA_OK;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s: cannot reserve %zu B of LDS: %s", what, bytes, hipGetErrorString(e));
    return VQA_E_UNSUPPORTED;
  }
  have = bytes;
  return VQA_OK;
}

int resident_per_cu(const void* fn, int threads, size_t lds) {
  static std::map<std::pair<const void*, size_t>, int> resident;
  std::lock_guard<std::mutex> lock(g_launch_mu);
  int& n = resident[{fn, lds}];
  if (n == 0 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, threads, lds) != hipSuccess || n < 1)) {
    (void)hipGetLastError();
    n = 1;
  }
  return n;
}

__global__ __launch_bounds__(256) void mse_kernel(const float* x, const float* r, const float* extra, float* dr,
                                                 long long n, float gscale, float* ws) {
  __shared__ float red[4];
  float part = 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float d = r[i] - x[i];
    part += d * d;
    float g = gscale * d;
    if (extra) g = g + extra[i];
    dr[i] = g;
  }
  const float s = block_sum_256(part, red);
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}

// float4 form (n % 4 == 0, 16-byte aligned buffers): two float4 of every buffer per thread and trip, both
// loaded before either is used (the second clamped to a valid index, its terms dropped past the end)
__global__ __launch_bounds__(256) void mse4_kernel(const float* x, const float* r, const float* extra, float* dr,
                                                  long long n4, float gscale, float* ws) {
  __shared__ float red[4];
  float part = 0.f;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += 2 * stride) {
    const long long j = i + stride < n4 ? i + stride : i;
    const f32x4 r0 = ((const f32x4*)r)[i], x0 = ((const f32x4*)x)[i];
    const f32x4 r1 = ((const f32x4*)r)[j], x1 = ((const f32x4*)x)[j];
    f32x4 e0 = {0.f, 0.f, 0.f, 0.f}, e1 = e0;
    if (extra) {
      e0 = ((const f32x4*)extra)[i];
      e1 = ((const f32x4*)extra)[j];
    }
    const f32x4 d0 = r0 - x0, d1 = r1 - x1;
    f32x4 g0 = gscale * d0, g1 = gscale * d1;
    if (extra) {
      g0 = g0 + e0;
      g1 = g1 + e1;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) part += d0[k] * d0[k];
    ((f32x4*)dr)[i] = g0;
    if (j != i) {
#pragma unroll
      for (int k = 0; k < 4; ++k) part += d1[k] * d1[k];
      ((f32x4*)dr)[j] = g1;
    }
  }
  const float s = block_sum_256(part, red);
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void mse_reduce_kernel(const float* ws, int n, float scale, float* out) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += ws[i];
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) out[0] = s * scale;
}

// The step's metric trackers (vqvae.py:262-304 update_metrics, VectorQuantizer.py:149-159) as one launch:
// macc rows [loss, recon, vqvae, spectral] then per level [level, recon, vq, spectral, batch_usage, usage,
// entropy], each (total, count). loss_slots = per level (recon, commit, spectral) sums over ranks, scaled by
// 1/world; the Python sums of the reference are left folds: level = (recon + commit) + spectral,
// total = ((0 + level_0) + level_1) + ...
// ok (nullable): the flag of a guarded step; a skipped step (ok[0] != 1) leaves every tracker row as it is, total
// and count.
__global__ void step_metrics_kernel(const float* loss_slots, const float* vqm, float* macc, int levels, float scale,
                                    const int* ok) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (ok && ok[0] != 1) return;
  float tot = 0.f, tr = 0.f, tc = 0.f, ts = 0.f;
  for (int l = 0; l < levels; ++l) {
    const float r = loss_slots[3 * l] * scale, c = loss_slots[3 * l + 1] * scale, sp = loss_slots[3 * l + 2] * scale;
    const float lv = (r + c) + sp;
    tot += lv;
    tr += r;
    tc += c;
    ts += sp;
    const float v[7] = {lv, r, c, sp, vqm[3 * l], vqm[3 * l + 1], vqm[3 * l + 2]};
    float* row = macc + 2 * (4 + 7 * l);
    for (int i = 0; i < 7; ++i) {
      row[2 * i] += v[i];
      row[2 * i + 1] += 1.f;
    }
  }
  const float g[4] = {tot, tr, tc, ts};
  for (int i = 0; i < 4; ++i) {
    macc[2 * i] += g[i];
    macc[2 * i + 1] += 1.f;
  }
}

// ---- on-device synthetic waveform feed (replaces the host-side chunk feed of
// data_utils.py:65-206 splitsongs / read_data and the notebook's tf.data pipeline) --------------------------
// x[b][t] = clip(0.5 sin(2 pi f_b t / sr + phi_b) + 0.05 eps, -1, 1), f_b ~ U[55, 2000) Hz, phi_b ~ U[0, 2 pi),
// eps ~ N(0, 1): every draw is a counter-based hash of (seed, rank, item, sample) — no state, any launch
// shape gives the same batch, ranks draw disjoint streams. The phase is reduced in fp64 (t up to 2^31).
__device__ __forceinline__ float u01(uint64_t h) { return (float)(h >> 40) * (1.0f / 16777216.0f); }  // [0, 1)
__device__ __forceinline__ uint64_t feed_key(uint64_t seed, int rank, long long item) {
  return splitmix64(splitmix64(seed ^ 0x5DEECE66DULL) + ((uint64_t)(unsigned)rank << 40) + (uint64_t)item);
}
__global__ __launch_bounds__(256) void synth_kernel(float* x, int B, long long T, uint64_t seed, int rank,
                                                   double inv_sr) {
  const int b = blockIdx.y;
  const uint64_t key = feed_key(seed, rank, b);
  const double f = 55.0 + (2000.0 - 55.0) * (double)u01(splitmix64(key ^ 1));
  const float ph = 6.2831853071795864f * u01(splitmix64(key ^ 2));
  const double cyc_per_sample = f * inv_sr;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < T; t += (long long)gridDim.x * 256) {
    double c = cyc_per_sample * (double)t;
    c -= floor(c);
    const float s = sinf(6.2831853071795864f * (float)c + ph);
    // Box-Muller from two independent hashes of (key, t)
    const uint64_t h = splitmix64(key + 0x9E3779B97F4A7C15ULL * (uint64_t)(t + 1));
    const float u1 = fmaxf(u01(h), 1.0f / 16777216.0f), u2 = u01(splitmix64(h));
    const float eps = sqrtf(-2.0f * logf(u1)) * cosf(6.2831853071795864f * u2);
    x[(long long)b * T + t] = fminf(fmaxf(0.5f * s + 0.05f * eps, -1.0f), 1.0f);
  }
}

}  // namespace vqa

using namespace vqa;

extern "C" const char* vqa_get_last_error(void) { return g_err; }
extern "C" const char* vqa_version(void) { return "libvqa 0.2 gfx950 abi 2"; }
extern "C" int vqa_abi_version(void) { return VQA_ABI_VERSION; }

extern "C" size_t vqa_mse_loss_workspace(int64_t n) { return n < 1 ? 0 : (size_t)blocks_for(n, 1024) * sizeof(float); }

extern "C" int vqa_mse_loss(const float* x, const float* r, const float* extra_grad, float* dr, float* loss_out,
                            int64_t n, void* workspace, size_t ws_bytes, vqa_stream_t stream) {
  VQA_ARG(x && r && dr && loss_out && n > 0, "mse_loss: bad arguments");
  const int nb = blocks_for(n, 1024);
  VQA_ARG(workspace && ws_bytes >= (size_t)nb * sizeof(float), "mse_loss: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const float inv_n = (float)(1.0 / (double)n);
  const float gscale = (float)(2.0 / (double)n);
  if (n % 4 == 0 && ((uintptr_t)x | (uintptr_t)r | (uintptr_t)extra_grad | (uintptr_t)dr) % 16 == 0) {
    hipLaunchKernelGGL(mse4_kernel, dim3(nb), dim3(256), 0, s, x, r, extra_grad, dr, (long long)(n / 4), gscale,
                       (float*)workspace);
    VQA_LAUNCHED("mse4_kernel");
  } else {
    hipLaunchKernelGGL(mse_kernel, dim3(nb), dim3(256), 0, s, x, r, extra_grad, dr, (long long)n, gscale,
                       (float*)workspace);
    VQA_LAUNCHED("mse_kernel");
  }
  hipLaunchKernelGGL(mse_reduce_kernel, dim3(1), dim3(256), 0, s, (const float*)workspace, nb, inv_n, loss_out);
  VQA_LAUNCHED("mse_reduce_kernel");
  return VQA_OK;
}

extern "C" int vqa_step_metrics(const float* loss_slots, const float* vq_metrics, float* macc, int levels, float scale,
                                vqa_stream_t stream) {
  VQA_ARG(loss_slots && vq_metrics && macc && levels > 0, "step_metrics: bad arguments");
  hipLaunchKernelGGL(step_metrics_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, loss_slots, vq_metrics, macc,
                     levels, scale, (const int*)nullptr);
  VQA_LAUNCHED("step_metrics_kernel");
  return VQA_OK;
}

extern "C" int vqa_step_metrics_if(const float* loss_slots, const float* vq_metrics, float* macc, int levels,
                                   float scale, const int32_t* ok, vqa_stream_t stream) {
  VQA_ARG(loss_slots && vq_metrics && macc && levels > 0, "step_metrics_if: bad arguments");
  VQA_ARG(ok, "step_metrics_if: null ok flag");
  hipLaunchKernelGGL(step_metrics_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, loss_slots, vq_metrics, macc,
                     levels, scale, ok);
  VQA_LAUNCHED("step_metrics_kernel");
  return VQA_OK;
}

extern "C" int vqa_synthetic_batch(float* x, int B, int64_t T, uint64_t seed, int rank, float sample_rate,
                                   vqa_stream_t stream) {
  VQA_ARG(x && B > 0 && T > 0 && B <= 65535 && sample_rate > 0.f, "synthetic_batch: bad arguments");
  const unsigned gx = (unsigned)std::min<long long>((T + 255) / 256, 1024);
  hipLaunchKernelGGL(synth_kernel, dim3(gx, (unsigned)B), dim3(256), 0, (hipStream_t)stream, x, B, (long long)T, seed,
                     rank, 1.0 / (double)sample_rate);
  VQA_LAUNCHED("synth_kernel");
  return VQA_OK;
}
