// vqa_resample.hip — polyphase sample-rate conversion of fp32 or int16 tracks (include/vqa.h: vqa_resample,
// vqa_resample_route). up = L, down = M, P taps per phase, W = P / 2: output m sits at input time m*M/L,
//   k0, r = divmod(m*M, L),  y[m] = sum_{i<P} x[k0 + i - W + 1] * T[r][i],  x zero outside [0, track_len).
// A workgroup of 256 threads computes a tile of consecutive outputs of one row, one output per thread: it stages the
// input span of the tile in LDS as fp32 (int16 scaled by 2^-15 there, zeros outside the track) and every thread
// walks its phase row in ascending i with one fmaf per tap, so an output's bits depend on (r, P) and its inputs only,
// never on the tile, m0 or B: a track resampled in chunks equals the track resampled whole.
// Two routes (resample_plan, shared by the launcher and vqa_resample_route):
//   table in LDS   rows at a stride of a multiple of 4 floats with stride / 4 odd, read 16 bytes at a time: the 16
//                  lanes of a ds_read_b128 group that hold rows distinct mod 16 touch distinct 4-bank slots (lanes
//                  of the same phase read one address, a broadcast)
//   table global   when table + staging exceed 160 KiB (coprime rates such as 22050 -> 16001: 16001 rows)
#include <algorithm>
#include <climits>

#include "vqa_common.h"
#include "vqa_launch.h"

namespace vqa {

constexpr int RS_THREADS = 256;
constexpr long long RS_LDS_LIMIT = 160 * 1024;   // what raise_dyn_lds can reserve; the kernel has no static LDS
constexpr long long RS_STAGE_LIMIT = 96 * 1024;  // the tile is halved until its input span fits this

struct ResamplePlan {
  int tile;        // outputs per workgroup (<= RS_THREADS)
  int stride;      // floats between the rows of the LDS table
  int span;        // floats of input staging: covers any tile of `tile` outputs
  int table_lds;   // 1: the table is staged in LDS
  long long lds;   // dynamic LDS bytes of the launch
};

// floats of input a tile of `tile` outputs can need: floor((m + tile - 1) M / L) - floor(m M / L) <= floor((tile - 1)
// M / L) + 1, plus the P taps of the last output
static long long span_of(int tile, int up, int down, int P) { return (long long)(tile - 1) * down / up + 1 + P; }

static ResamplePlan resample_plan(int up, int down, int P) {
  ResamplePlan p;
  p.tile = RS_THREADS;
  while (p.tile > 1 && span_of(p.tile, up, down, P) * 4 > RS_STAGE_LIMIT) p.tile /= 2;
  p.span = (int)span_of(p.tile, up, down, P);  // tile 1: P + 1 <= 8193 floats
  p.stride = (P + 3) / 4 * 4;
  if ((p.stride / 4) % 2 == 0) p.stride += 4;
  const long long table = (long long)up * p.stride * 4;
  p.table_lds = table + (long long)p.span * 4 <= RS_LDS_LIMIT;
  p.lds = (long long)p.span * 4 + (p.table_lds ? table : 0);
  return p;
}

// grid (tiles, B). lds: [table, up * stride floats, when TAB][staging, span floats]
template <bool TAB, bool I16>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const void* __restrict__ x, long long ldx, long long in0,
                                                              long long n_in, long long track_len,
                                                              float* __restrict__ out, long long ldo, long long m0,
                                                              long long n_out, int up, int down,
                                                              const float* __restrict__ taps, int P, int stride,
                                                              int tile) {
  extern __shared__ __align__(16) float rs_lds[];
  float* tab = rs_lds;
  float* xs = rs_lds + (TAB ? up * stride : 0);
  const int tid = threadIdx.x, b = blockIdx.y, W = P / 2;
  const long long t0 = (long long)blockIdx.x * tile;  // first output of the tile, relative to m0
  const int nt = (int)(n_out - t0 < tile ? n_out - t0 : tile);
  const long long mfirst = m0 + t0;
  const long long kfirst = mfirst * down / up, klast = (mfirst + nt - 1) * down / up;
  const long long k_lo = kfirst - W + 1;       // track index of xs[0]
  const int span = (int)(klast - kfirst) + P;  // <= the plan's span
  if (TAB) {
    const int total = up * P;
    for (int idx = tid; idx < total; idx += RS_THREADS) {
      const int r = idx / P, i = idx - r * P;
      tab[r * stride + i] = taps[idx];
    }
  }
  for (int s = tid; s < span; s += RS_THREADS) {
    const long long k = k_lo + s, j = k - in0;
    float v = 0.0f;
    if (k >= 0 && k < track_len && j >= 0 && j < n_in) {
      if (I16)
        v = (float)((const int16_t*)x)[(long long)b * ldx + j] * 0.000030517578125f;  // 2^-15, exact
      else
        v = ((const float*)x)[(long long)b * ldx + j];
    }
    xs[s] = v;
  }
  __syncthreads();
  if (tid >= nt) return;
  const long long md = (mfirst + tid) * down, k0 = md / up;
  const int r = (int)(md - k0 * up);
  const float* xp = xs + (int)(k0 - kfirst);  // xp[i] = x[k0 + i - W + 1]
  float acc = 0.0f;
  int i = 0;
  if (TAB) {
    const float* tp = tab + r * stride;
    for (; i + 4 <= P; i += 4) {
      const f32x4 t = *(const f32x4*)(tp + i);
      acc = fmaf(xp[i], t[0], acc);
      acc = fmaf(xp[i + 1], t[1], acc);
      acc = fmaf(xp[i + 2], t[2], acc);
      acc = fmaf(xp[i + 3], t[3], acc);
    }
    for (; i < P; ++i) acc = fmaf(xp[i], tp[i], acc);
  } else {
    const float* tp = taps + (long long)r * P;
    for (; i < P; ++i) acc = fmaf(xp[i], tp[i], acc);
  }
  out[(long long)b * ldo + t0 + tid] = acc;
}

static int gcd_int(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// the checks vqa_resample and vqa_resample_route share
static int resample_check_rates(int up, int down, int P) {
  VQA_ARG(up >= 1 && down >= 1, "resample: up %d and down %d must be positive", up, down);
  VQA_ARG(gcd_int(up, down) == 1, "resample: up %d and down %d are not coprime", up, down);
  VQA_ARG(P >= 2 && P <= 8192 && P % 2 == 0, "resample: taps_per_phase %d is not even and in [2, 8192]", P);
  return VQA_OK;
}

template <bool TAB, bool I16>
static int launch_resample(const ResamplePlan& p, const void* x, long long ldx, long long in0, long long n_in,
                           long long track_len, float* out, long long ldo, long long m0, long long n_out, int B,
                           int up, int down, const float* taps, int P, hipStream_t s) {
  const void* fn = (const void*)resample_kernel<TAB, I16>;
  if (p.lds > 64 * 1024) {
    const int rc = raise_dyn_lds(fn, (size_t)p.lds, "resample");
    if (rc != VQA_OK) return rc;
  }
  const dim3 grid((unsigned)((n_out - 1) / p.tile + 1), (unsigned)B), block(RS_THREADS);
  hipLaunchKernelGGL((resample_kernel<TAB, I16>), grid, block, (size_t)p.lds, s, x, ldx, in0, n_in, track_len, out, ldo,
                     m0, n_out, up, down, taps, P, p.stride, p.tile);
  VQA_LAUNCHED("resample_kernel");
  return VQA_OK;
}

}  // namespace vqa

using namespace vqa;

extern "C" int vqa_resample_route(int up, int down, int taps_per_phase, int* table_in_lds, int* tile_outputs) {
  VQA_ARG(table_in_lds && tile_outputs, "resample: null table_in_lds or tile_outputs");
  const int rc = resample_check_rates(up, down, taps_per_phase);
  if (rc != VQA_OK) return rc;
  const ResamplePlan p = resample_plan(up, down, taps_per_phase);
  *table_in_lds = p.table_lds;
  *tile_outputs = p.tile;
  return VQA_OK;
}

extern "C" int vqa_resample(const void* x, int x_dtype, int64_t ldx, int64_t in0, int64_t n_in, int64_t track_len,
                            float* out, int64_t ldo, int64_t m0, int64_t n_out, int B, int up, int down,
                            const float* taps, int taps_per_phase, vqa_stream_t stream) {
  typedef long long ll;
  const int P = taps_per_phase, W = P / 2;
  VQA_ARG(x && out && taps, "resample: null x, out or taps");
  VQA_ARG(B >= 1 && B <= 65535, "resample: B %d outside [1, 65535]", B);
  const int rc = resample_check_rates(up, down, P);
  if (rc != VQA_OK) return rc;
  VQA_ARG(x_dtype == 0 || x_dtype == 1, "resample: x_dtype %d is neither 0 (fp32) nor 1 (int16)", x_dtype);
  VQA_ARG((uintptr_t)x % (x_dtype == 0 ? 4 : 2) == 0, "resample: x is not %d-byte aligned", x_dtype == 0 ? 4 : 2);
  VQA_ARG((uintptr_t)out % 4 == 0, "resample: out is not 4-byte aligned");
  VQA_ARG((uintptr_t)taps % 4 == 0, "resample: taps is not 4-byte aligned");
  VQA_ARG(n_out > 0 && track_len > 0, "resample: n_out %lld and track_len %lld must be positive", (ll)n_out,
          (ll)track_len);
  VQA_ARG(m0 >= 0 && in0 >= 0 && n_in >= 0, "resample: negative m0 %lld, in0 %lld or n_in %lld", (ll)m0, (ll)in0,
          (ll)n_in);
  const __int128 total = ((__int128)track_len * up + down - 1) / down;  // ceil(track_len L / M)
  VQA_ARG((__int128)m0 + n_out <= total, "resample: outputs [%lld, %lld + %lld) exceed the track's %lld outputs",
          (ll)m0, (ll)m0, (ll)n_out, (ll)(total > LLONG_MAX ? LLONG_MAX : (ll)total));
  VQA_ARG(ldx >= n_in, "resample: ldx %lld below n_in %lld", (ll)ldx, (ll)n_in);
  VQA_ARG(ldo >= n_out, "resample: ldo %lld below n_out %lld", (ll)ldo, (ll)n_out);
  ll prod;
  VQA_ARG(!__builtin_mul_overflow((ll)(m0 + n_out), (ll)down, &prod),
          "resample: (m0 + n_out) * down = %lld * %d does not fit in int64", (ll)(m0 + n_out), down);
  VQA_ARG(in0 <= LLONG_MAX - n_in, "resample: in0 %lld + n_in %lld does not fit in int64", (ll)in0, (ll)n_in);
  // the input the outputs need, inside the track: never empty (every output's k0 lies in [0, track_len))
  const ll lo = std::max<ll>((ll)m0 * down / up - W + 1, 0);
  const ll hi = std::min<ll>((ll)(m0 + n_out - 1) * down / up + W, (ll)track_len - 1);
  VQA_ARG(in0 <= lo && hi < in0 + n_in,
          "resample: the outputs need input samples [%lld, %lld], the call holds [%lld, %lld)", lo, hi, (ll)in0,
          (ll)(in0 + n_in));
  const ResamplePlan p = resample_plan(up, down, P);
  VQA_ARG((n_out - 1) / p.tile + 1 <= INT_MAX, "resample: n_out %lld needs more than 2^31 - 1 tiles of %d",
          (ll)n_out, p.tile);
  hipStream_t s = (hipStream_t)stream;
#define RS_GO(TAB, I16) \
  launch_resample<TAB, I16>(p, x, ldx, in0, n_in, track_len, out, ldo, m0, n_out, B, up, down, taps, P, s)
  if (p.table_lds) return x_dtype ? RS_GO(true, true) : RS_GO(true, false);
  return x_dtype ? RS_GO(false, true) : RS_GO(false, false);
#undef RS_GO
}
