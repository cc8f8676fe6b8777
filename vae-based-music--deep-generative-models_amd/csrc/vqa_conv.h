// vqa_conv.h — what the three conv translation units share (internal): the gather and weight-gradient argument
// blocks, the host plans and routes, and the entry points vqa_conv.hip calls.
//   vqa_conv_gather.hip : the gather kernels (forward and data gradient), their plans and run_gather
//   vqa_conv_wgrad.hip  : the weight-gradient kernels, the partial-sum reducers, their plan and run_wgrad
//   vqa_conv.hip        : the C ABI (no kernel): argument builders, entry points, vqa_conv1d_route
//
// Replaces the TF ops behind keras Conv1D / Conv1DTranspose on the reference's hot path:
//   resnet.py:13,17 (dilated residual convs), encdec.py:33 (strided down conv), :38 (projection),
//   :60 (decoder pre-conv), :67-68 (Conv1DTranspose up conv), :148 (decoder output conv).
//
// Every forward and data-gradient is ONE "gather" convolution
//     y[n, t, o] = sum_{k, c} act(x[n, t*S + k*D - P, c]) * Weff[k][c][o]      (+bias, mask, residual)
// with three ways of reading the fp32 Keras weight ("wmode"):
//   DIRECT : Weff = W[k][c][o]                       conv fwd; conv-transpose data-grad (stride 2)
//   FLIP_T : Weff = W[Kb-1-k][o][c]                  stride-1 conv data-grad
//   PAIR   : out pair j holds full rows 2j, 2j+1:    conv-transpose fwd; stride-2 conv data-grad
//            Weff[a+1][c][p*Ob+ob] = W[p + Pb - 2a][ob][c]  (a in {-1,0,1}, zero when out of range)
// so the MFMA gather kernel covers all of them; the PAIR layout (n, j, p, ob) is exactly the NTC
// layout of the full-resolution tensor. Weight gradients are split-row MFMA reductions with
// per-workgroup fp32 partials and a deterministic second pass.
#pragma once
#include "vqa_common.h"

namespace vqa {

enum { W_DIRECT = 0, W_FLIP_T = 1, W_PAIR = 2 };

struct GatherArgs {
  const void* x;
  const float* w;
  const float* bias;
  const void* resid;
  const void* mask;
  void* y;
  int B, T_in, T_out;  // x rows per item, gather-output rows per item
  int C, O;            // gather input / output channels
  int K, S, D, P;      // gather taps, stride, dilation, left pad
  int wmode, Kb, Pb;   // weight mapping; base taps; base pad (PAIR)
  int T_full;          // PAIR: full-resolution rows per item (store guard)
  int flags;
  // fused weight gradient (stride-1 data-gradient only): `mask` is the conv input u (always staged),
  // wpart receives one fp32 partial [K*O*C dW | C db] per workgroup, wrelu: dW uses relu(u)
  float* wpart = nullptr;
  int wrelu = 0;
  // generic kernel only: take the weights rounded to bf16, as the MFMA kernels stage them (run_gather sets it for
  // the all-bf16 convs whose channel counts the MFMA kernel serves and whose tile is too large for it)
  int wbf16 = 0;
};

__device__ __forceinline__ float weff(const GatherArgs& a, int k, int c, int o) {
  if (a.wmode == W_DIRECT) return a.w[((size_t)k * a.C + c) * a.O + o];
  if (a.wmode == W_FLIP_T) return a.w[((size_t)(a.Kb - 1 - k) * a.O + o) * a.C + c];
  const int Ob = a.O >> 1;
  const int p = o >= Ob ? 1 : 0;
  const int ob = o - p * Ob;
  const int kb = p + a.Pb - 2 * (k - 1);
  return (kb >= 0 && kb < a.Kb) ? a.w[((size_t)kb * Ob + ob) * a.C + c] : 0.f;
}

// output element index (n, t, o) -> linear offset in y / resid / mask, or -1 if outside (PAIR tail)
__device__ __forceinline__ long long out_index(const GatherArgs& a, int n, int t, int o) {
  if (a.wmode == W_PAIR) {
    const int Ob = a.O >> 1;
    const int p = o >= Ob ? 1 : 0;
    const int u = 2 * t + p;
    if (u >= a.T_full) return -1;
    return ((long long)n * a.T_full + u) * Ob + (o - p * Ob);
  }
  return ((long long)n * a.T_out + t) * a.O + o;
}

__device__ __forceinline__ int bias_index(const GatherArgs& a, int o) {
  return a.wmode == W_PAIR ? (o >= (a.O >> 1) ? o - (a.O >> 1) : o) : o;
}

// ---- raw buffer access, used by the kernels of both files: one item's rows as a buffer resource, so the hardware
// range check zero-fills loads and drops stores outside the item
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef short s16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t item_rsrc(const void* base, long long off, unsigned bytes) {
  const unsigned long long p = (unsigned long long)base + (unsigned long long)off;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)p);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(p >> 32));
  void* q = (void*)(((unsigned long long)hi << 32) | lo);
  return __builtin_amdgcn_make_buffer_rsrc(q, (short)0, (int)__builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}

// x-row byte offset that stays out of range after adding any tile base (|base| < 2^30)
constexpr int kOOB = -0x40000000;

// ------------------------------------------------------------------------------------------------
// Weight gradient: dW[k][c][o] = sum_{n,t} act(x[n, t*S + k*D - P, c]) * g[n, t, o],
// db[o] = sum_{n,t} g[n, t, o]. Grid = (chunks per item, items); each workgroup reduces CH output
// rows in TT-row sub-tiles staged in LDS and writes fp32 partials [wg][K*C*O + O]; a second
// kernel sums the partials in a fixed order (deterministic).
struct WgradArgs {
  const void* x;
  const void* g;
  float* ws;
  int B, T_in, T_out, C, O, K, S, D, P;
  int CH, nchunk;
  int flags;  // VQA_PRE_RELU, VQA_X_F32, VQA_Y_F32, WG_DB_FROM_X
  int nb;     // bias entries per partial: O (bias = column sums of g) or C (WG_DB_FROM_X)
};

// bias gradient = column sums of the INPUT x over the rows this workgroup owns (conv-transpose bias:
// its output-gradient is the gather input of the weight gradient)
constexpr int WG_DB_FROM_X = 1 << 8;

// resident workgroups per CU the persistent grid assumes at most (also bounds the fused-wgrad partials)
constexpr int kMaxGatherPerCU = 4;

// What the MFMA gather kernel needs for one launch, from the shape alone (no HIP call): the tile rows, the 16-byte
// chunks per thread of the register stager (PV: 3, 4, 5, 8 or 12) and the dynamic LDS. ok = false: this conv does
// not run on the MFMA kernel (run_gather then takes the next kernel down the list).
struct MfmaPlan {
  bool ok;
  int tm, pv, nep;
  size_t lds;
};

// Which kernel a gather conv runs, decided on the host from the shape, dtype and flags alone (no HIP call): the
// one list run_gather launches from and vqa_conv1d_route reports from.
enum { G_CONV32, G_MFMA, G_CI1, G_THINO, G_THIN, G_DIRECT };
struct GatherRoute {
  int family;
  int pvx;     // G_CONV32: x chunks per thread
  MfmaPlan m;  // G_MFMA
};

// ---- weight gradient planning ----
enum { WG_MFMA = 0, WG_THIN_X = 1, WG_THIN_G = 2, WG_DIRECT = 3 };
struct WgradPlan {
  int kind;
  int TT, CH, nchunk, nwg, E, nb;
  size_t lds, ws_bytes;
};

// ---- vqa_conv_gather.hip
int gather_check(const GatherArgs& a, int dtype);  // the shape checks of every gather conv (pointers apart)
GatherRoute gather_route(const GatherArgs& a, int dtype);
int gather_nep(const GatherArgs& a, bool fw);  // epilogue tiles staged per tile (fw: the fused weight gradient's)
bool gather_thin_fits(const GatherArgs& a);
int conv32_pvx(const GatherArgs& a, int dtype, bool fw);  // x chunks per thread of the 32-channel kernel, 0: n/a
int run_gather(const GatherArgs& a, int dtype, hipStream_t s);
// the 32-channel kernel with the fused weight gradient (a.wpart set); *nwg = its workgroups = partial rows
int launch_conv32_fused(const GatherArgs& a, int pvx, int dtype, hipStream_t s, int* nwg);

// ---- vqa_conv_wgrad.hip
int wgrad_route(WgradPlan* out, int dtype, int B, int T_in, int T_out, int C, int O, int K, int S, int D, int flags);
int run_wgrad(const void* x, const void* g, float* dw, float* db, int B, int T_in, int T_out, int C, int O, int K,
              int S, int D, int P, int flags, int dtype, void* ws, size_t ws_bytes, hipStream_t s,
              vqa_partials_desc* defer);
size_t wgrad_ws(int dtype, int B, int T_in, int T_out, int C, int O, int K, int S, int D, int flags);
// dw[e] = sum_p ws[p*E + e] for e < n_w, db[e - n_w] beyond: one launch, fixed summation order
int reduce_partials(const float* ws, int nparts, int E, int n_w, float* dw, float* db, hipStream_t s);

}  // namespace vqa
