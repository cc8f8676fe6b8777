// vqa_conv.hip — the C ABI of the 1-D convolutions (host only; the kernels are in vqa_conv_gather.hip,
// vqa_conv_wgrad.hip and vqa_conv_ends.hip): "same" padding, the gather each entry point runs, the entry points, and
// vqa_conv1d_route, which reports the kernel a call would run from the same routing functions.
#include "vqa_conv.h"
#include "vqa_launch.h"
#include <algorithm>

using namespace vqa;

// -1 for a shape TF's "same" padding does not define (stride or dilation < 1, K < 1, T_in < 0)
extern "C" int vqa_same_out_len(int T_in, int stride) {
  if (stride < 1 || T_in < 0) return -1;
  return (T_in + stride - 1) / stride;
}
extern "C" int vqa_same_pad_left(int T_in, int K, int stride, int dilation) {
  if (stride < 1 || dilation < 1 || K < 1 || T_in < 0) return -1;
  const int out = (T_in + stride - 1) / stride;
  const int pad = std::max((out - 1) * stride + (K - 1) * dilation + 1 - T_in, 0);
  return pad / 2;
}

// ---- the gather each conv entry point runs (the entry points launch it, vqa_conv1d_route reports its kernel)
static GatherArgs conv_fwd_gather(const void* x, const float* w, const float* bias, const void* residual, void* y,
                                  int B, int T_in, int T_out, int C_in, int C_out, int K, int stride, int dilation,
                                  int pad_left, int flags) {
  return GatherArgs{x, w, bias, residual, nullptr, y, B, T_in, T_out, C_in, C_out, K, stride, dilation, pad_left,
                    W_DIRECT, K, 0, T_out, flags & (VQA_PRE_RELU | VQA_ADD_RESIDUAL | VQA_X_F32 | VQA_Y_F32)};
}

// flags for the data-gradient gather: the gather input is dy (y side), output dx (x side)
static int swap_xy_flags(int flags) {
  int f = flags & (VQA_POST_MASK | VQA_ADD_RESIDUAL);
  if (flags & VQA_X_F32) f |= VQA_Y_F32;
  if (flags & VQA_Y_F32) f |= VQA_X_F32;
  return f;
}

static int conv_bwd_data_gather(GatherArgs* out, const void* dy, const float* w, const void* mask,
                                const void* residual, void* dx, int B, int T_in, int T_out, int C_in, int C_out,
                                int K, int stride, int dilation, int pad_left, int flags) {
  const int f = swap_xy_flags(flags);
  if (stride == 1) {
    *out = GatherArgs{dy, w, nullptr, residual, mask, dx, B, T_out, T_in, C_out, C_in, K, 1, dilation,
                      (K - 1) * dilation - pad_left, W_FLIP_T, K, 0, T_in, f};
    return VQA_OK;
  }
  VQA_REQUIRE(stride == 2 && K == 4 && dilation == 1 && pad_left == 1, VQA_E_UNSUPPORTED,
              "conv1d_bwd_data: strided data-gradient supports stride 2, K 4, pad_left 1 (got s=%d K=%d d=%d p=%d)",
              stride, K, dilation, pad_left);
  *out = GatherArgs{dy, w, nullptr, residual, mask, dx, B, T_out, T_out, C_out, 2 * C_in, 3, 1, 1, 1,
                    W_PAIR, K, pad_left, T_in, f};
  return VQA_OK;
}

static int convT_check(int K, int stride, int pad_left) {
  VQA_REQUIRE(stride == 2 && K == 4 && pad_left == 1, VQA_E_UNSUPPORTED,
              "conv1d_transpose: supports stride 2, K 4, pad_left 1 (got s=%d K=%d p=%d)", stride, K, pad_left);
  return VQA_OK;
}

static GatherArgs convT_fwd_gather(const void* x, const float* w, const float* bias, const void* residual, void* y,
                                   int B, int T_in, int T_out, int C_in, int C_out, int K, int pad_left, int flags) {
  return GatherArgs{x, w, bias, residual, nullptr, y, B, T_in, T_in, C_in, 2 * C_out, 3, 1, 1, 1,
                    W_PAIR, K, pad_left, T_out, flags & (VQA_PRE_RELU | VQA_ADD_RESIDUAL | VQA_X_F32 | VQA_Y_F32)};
}

static GatherArgs convT_bwd_data_gather(const void* dy, const float* w, const void* mask, const void* residual,
                                        void* dx, int B, int T_in, int T_out, int C_in, int C_out, int K, int stride,
                                        int pad_left, int flags) {
  return GatherArgs{dy, w, nullptr, residual, mask, dx, B, T_out, T_in, C_out, C_in, K, stride, 1, pad_left,
                    W_DIRECT, K, 0, T_in, swap_xy_flags(flags)};
}

// flags the weight gradient of a conv keeps
static int conv_wgrad_flags(int flags) { return flags & (VQA_PRE_RELU | VQA_X_F32 | VQA_Y_F32); }
// flags of the gather weight-gradient a transposed conv's weight gradient runs (dy is its input)
static int convT_wgrad_flags(int flags) { return (swap_xy_flags(flags) & (VQA_X_F32 | VQA_Y_F32)) | WG_DB_FROM_X; }

extern "C" int vqa_conv1d_fwd(const void* x, const float* w, const float* bias, const void* residual, void* y, int B,
                              int T_in, int T_out, int C_in, int C_out, int K, int stride, int dilation, int pad_left,
                              int flags, int dtype, vqa_stream_t stream) {
  VQA_ARG(stride >= 1 && dilation >= 1 && K >= 1, "conv1d_fwd: stride %d, dilation %d, K %d must be >= 1", stride,
          dilation, K);
  VQA_ARG(T_out == (T_in + stride - 1) / stride, "conv1d_fwd: T_out %d != ceil(T_in/stride)", T_out);
  if (co1_supported(C_in, C_out, K, stride, dilation, dtype, flags) && (dtype == VQA_F32 || dtype == VQA_BF16)) {
    VQA_ARG(x && w && y && B > 0 && T_in > 0, "conv1d_fwd: bad arguments");
    VQA_ARG(!(flags & VQA_ADD_RESIDUAL) || residual, "VQA_ADD_RESIDUAL without residual");
    return co1_fwd(x, w, bias, residual, y, B, T_in, C_in, K, dilation, pad_left,
                   flags & (VQA_PRE_RELU | VQA_ADD_RESIDUAL | VQA_X_F32 | VQA_Y_F32), dtype, (hipStream_t)stream);
  }
  const GatherArgs a = conv_fwd_gather(x, w, bias, residual, y, B, T_in, T_out, C_in, C_out, K, stride, dilation,
                                       pad_left, flags);
  return run_gather(a, dtype, (hipStream_t)stream);
}

extern "C" int vqa_conv1d_bwd_data(const void* dy, const float* w, const void* mask, const void* residual, void* dx,
                                   int B, int T_in, int T_out, int C_in, int C_out, int K, int stride, int dilation,
                                   int pad_left, int flags, int dtype, vqa_stream_t stream) {
  VQA_ARG(stride >= 1 && dilation >= 1 && K >= 1, "conv1d_bwd_data: stride %d, dilation %d, K %d must be >= 1", stride,
          dilation, K);
  VQA_ARG(T_out == (T_in + stride - 1) / stride, "conv1d_bwd_data: T_out %d != ceil(T_in/stride)", T_out);
  if (co1_supported(C_in, C_out, K, stride, dilation, dtype, flags) && (dtype == VQA_F32 || dtype == VQA_BF16)) {
    VQA_ARG(dy && w && dx && B > 0 && T_in > 0, "conv1d_bwd_data: bad arguments");
    VQA_ARG(!(flags & VQA_POST_MASK) || mask, "VQA_POST_MASK without mask");
    VQA_ARG(!(flags & VQA_ADD_RESIDUAL) || residual, "VQA_ADD_RESIDUAL without residual");
    // same kernel (and dx arithmetic) as the fused data + weight gradient, without the weight partials
    const int f = ((flags & VQA_POST_MASK) ? VQA_PRE_RELU : 0) | (flags & (VQA_ADD_RESIDUAL | VQA_X_F32 | VQA_Y_F32));
    return co1_bwd(dy, w, (flags & VQA_POST_MASK) ? mask : nullptr, residual, dx, B, T_in, C_in, K, dilation,
                   pad_left, f, dtype, nullptr, nullptr, (hipStream_t)stream);
  }
  GatherArgs a{};
  const int rc = conv_bwd_data_gather(&a, dy, w, mask, residual, dx, B, T_in, T_out, C_in, C_out, K, stride, dilation,
                                      pad_left, flags);
  if (rc != VQA_OK) return rc;
  return run_gather(a, dtype, (hipStream_t)stream);
}

extern "C" size_t vqa_conv1d_bwd_weight_workspace(int B, int T_in, int T_out, int C_in, int C_out, int K, int stride,
                                                  int dilation, int pad_left, int flags, int dtype) {
  (void)pad_left;
  return wgrad_ws(dtype, B, T_in, T_out, C_in, C_out, K, stride, dilation, flags);
}

extern "C" int vqa_conv1d_bwd_weight(const void* x, const void* dy, float* dw, float* db, int B, int T_in, int T_out,
                                     int C_in, int C_out, int K, int stride, int dilation, int pad_left, int flags,
                                     int dtype, void* workspace, size_t ws_bytes, vqa_stream_t stream) {
  VQA_ARG(stride >= 1 && dilation >= 1 && K >= 1, "conv1d_bwd_weight: stride %d, dilation %d, K %d must be >= 1", stride,
          dilation, K);
  VQA_ARG(T_out == (T_in + stride - 1) / stride, "conv1d_bwd_weight: T_out %d != ceil(T_in/stride)", T_out);
  return run_wgrad(x, dy, dw, db, B, T_in, T_out, C_in, C_out, K, stride, dilation, pad_left,
                   conv_wgrad_flags(flags), dtype, workspace, ws_bytes, (hipStream_t)stream,
                   nullptr);
}

extern "C" int vqa_conv1d_transpose_fwd(const void* x, const float* w, const float* bias, const void* residual,
                                        void* y, int B, int T_in, int T_out, int C_in, int C_out, int K, int stride,
                                        int pad_left, int flags, int dtype, vqa_stream_t stream) {
  if (const int rc = convT_check(K, stride, pad_left)) return rc;
  VQA_ARG(T_out == stride * T_in, "conv1d_transpose_fwd: T_out %d != stride*T_in", T_out);
  const GatherArgs a = convT_fwd_gather(x, w, bias, residual, y, B, T_in, T_out, C_in, C_out, K, pad_left, flags);
  return run_gather(a, dtype, (hipStream_t)stream);
}

extern "C" int vqa_conv1d_transpose_bwd_data(const void* dy, const float* w, const void* mask, const void* residual,
                                             void* dx, int B, int T_in, int T_out, int C_in, int C_out, int K,
                                             int stride, int pad_left, int flags, int dtype, vqa_stream_t stream) {
  if (const int rc = convT_check(K, stride, pad_left)) return rc;
  VQA_ARG(T_out == stride * T_in, "conv1d_transpose_bwd_data: T_out %d != stride*T_in", T_out);
  const GatherArgs a = convT_bwd_data_gather(dy, w, mask, residual, dx, B, T_in, T_out, C_in, C_out, K, stride,
                                             pad_left, flags);
  return run_gather(a, dtype, (hipStream_t)stream);
}

extern "C" size_t vqa_conv1d_transpose_bwd_weight_workspace(int B, int T_in, int T_out, int C_in, int C_out, int K,
                                                            int stride, int pad_left, int flags, int dtype) {
  (void)pad_left;
  const int f = convT_wgrad_flags(flags);
  return wgrad_ws(dtype, B, T_out, T_in, C_out, C_in, K, stride, 1, f);
}

extern "C" int vqa_conv1d_transpose_bwd_weight(const void* x, const void* dy, float* dw, float* db, int B, int T_in,
                                               int T_out, int C_in, int C_out, int K, int stride, int pad_left,
                                               int flags, int dtype, void* workspace, size_t ws_bytes,
                                               vqa_stream_t stream) {
  if (const int rc = convT_check(K, stride, pad_left)) return rc;
  VQA_ARG(T_out == stride * T_in, "conv1d_transpose_bwd_weight: T_out %d != stride*T_in", T_out);
  // dW[k][co][ci] = sum_i dy[2i + k - 1][co] * x[i][ci]: the gather weight-gradient with dy as its input;
  // db[co] = column sums of dy, taken from the same staged rows (WG_DB_FROM_X)
  const int f = convT_wgrad_flags(flags);
  return run_wgrad(dy, x, dw, db, B, T_out, T_in, C_out, C_in, K, stride, 1, pad_left, f, dtype, workspace, ws_bytes,
                   (hipStream_t)stream, nullptr);
}

extern "C" int vqa_conv1d_bwd_weight_partials(const void* x, const void* dy, float* dw, float* db, int B, int T_in,
                                              int T_out, int C_in, int C_out, int K, int stride, int dilation,
                                              int pad_left, int flags, int dtype, void* workspace, size_t ws_bytes,
                                              vqa_partials_desc* desc, vqa_stream_t stream) {
  VQA_ARG(desc, "bwd_weight_partials: NULL descriptor");
  VQA_ARG(stride >= 1 && dilation >= 1 && K >= 1, "conv1d_bwd_weight: stride %d, dilation %d, K %d must be >= 1", stride,
          dilation, K);
  VQA_ARG(T_out == (T_in + stride - 1) / stride, "conv1d_bwd_weight: T_out %d != ceil(T_in/stride)", T_out);
  return run_wgrad(x, dy, dw, db, B, T_in, T_out, C_in, C_out, K, stride, dilation, pad_left,
                   conv_wgrad_flags(flags), dtype, workspace, ws_bytes, (hipStream_t)stream,
                   desc);
}

extern "C" int vqa_conv1d_transpose_bwd_weight_partials(const void* x, const void* dy, float* dw, float* db, int B,
                                                        int T_in, int T_out, int C_in, int C_out, int K, int stride,
                                                        int pad_left, int flags, int dtype, void* workspace,
                                                        size_t ws_bytes, vqa_partials_desc* desc,
                                                        vqa_stream_t stream) {
  VQA_ARG(desc, "bwd_weight_partials: NULL descriptor");
  if (const int rc = convT_check(K, stride, pad_left)) return rc;
  VQA_ARG(T_out == stride * T_in, "conv1d_transpose_bwd_weight: T_out %d != stride*T_in", T_out);
  const int f = convT_wgrad_flags(flags);
  return run_wgrad(dy, x, dw, db, B, T_out, T_in, C_out, C_in, K, stride, 1, pad_left, f, dtype, workspace, ws_bytes,
                   (hipStream_t)stream, desc);
}

// ---- fused data + weight gradient of a stride-1 conv whose input u feeds it through an optional ReLU
static size_t fused_bwd_ws(int C_in, int C_out, int K) {
  return (size_t)cu_count() * kMaxGatherPerCU * (size_t)(K * C_in * C_out + C_out) * sizeof(float);
}

static GatherArgs fused_bwd_args(const void* dy, const float* w, const void* x, const void* residual, void* dx, int B,
                                 int T_in, int T_out, int C_in, int C_out, int K, int dilation, int pad_left,
                                 int flags) {
  const bool relu = flags & VQA_PRE_RELU;
  const int f = swap_xy_flags(flags & (VQA_ADD_RESIDUAL | VQA_X_F32 | VQA_Y_F32)) | (relu ? VQA_POST_MASK : 0);
  GatherArgs a{dy, w, nullptr, residual, x, dx, B, T_out, T_in, C_out, C_in, K, 1, dilation,
               (K - 1) * dilation - pad_left, W_FLIP_T, K, 0, T_in, f};
  a.wrelu = relu ? 1 : 0;
  return a;
}

// how vqa_conv1d_bwd_data_weight runs: the one-output-channel kernel, the 32-channel kernel with the fused weight
// gradient (*pvx = its x chunks per thread), or the data gradient followed by the weight gradient
enum { F_CO1, F_CONV32, F_TWO_CALL };
static int fused_route(int B, int T_in, int T_out, int C_in, int C_out, int K, int stride, int dilation, int pad_left,
                       int flags, int dtype, int* pvx) {
  *pvx = 0;
  if (co1_supported(C_in, C_out, K, stride, dilation, dtype, flags)) return F_CO1;
  if (stride == 1) {
    const GatherArgs a = fused_bwd_args(nullptr, nullptr, nullptr, nullptr, nullptr, B, T_in, T_out, C_in, C_out, K,
                                        dilation, pad_left, flags);
    if ((*pvx = conv32_pvx(a, dtype, true))) return F_CONV32;
  }
  return F_TWO_CALL;
}

// the flags of the two calls of the fallback
static int two_call_data_flags(int flags) {
  return ((flags & VQA_PRE_RELU) ? VQA_POST_MASK : 0) | (flags & (VQA_ADD_RESIDUAL | VQA_X_F32 | VQA_Y_F32));
}

extern "C" size_t vqa_conv1d_bwd_data_weight_workspace(int B, int T_in, int T_out, int C_in, int C_out, int K,
                                                       int stride, int dilation, int pad_left, int flags, int dtype) {
  if (B < 1 || T_in < 1 || T_out < 1 || C_in < 1 || C_out < 1 || K < 1 || stride < 1 || dilation < 1) return 0;
  size_t need = wgrad_ws(dtype, B, T_in, T_out, C_in, C_out, K, stride, dilation, conv_wgrad_flags(flags));
  int pvx = 0;
  const int route = fused_route(B, T_in, T_out, C_in, C_out, K, stride, dilation, pad_left, flags, dtype, &pvx);
  if (route == F_CO1) need = std::max(need, co1_bwd_workspace(C_in, K));
  if (route == F_CONV32) need = std::max(need, fused_bwd_ws(C_in, C_out, K));
  return need;
}

extern "C" int vqa_conv1d_bwd_data_weight(const void* dy, const float* w, const void* x, const void* residual,
                                          void* dx, float* dw, float* db, int B, int T_in, int T_out, int C_in,
                                          int C_out, int K, int stride, int dilation, int pad_left, int flags,
                                          int dtype, void* workspace, size_t ws_bytes, vqa_partials_desc* desc,
                                          vqa_stream_t stream) {
  VQA_ARG(stride >= 1 && dilation >= 1 && K >= 1, "conv1d_bwd_data_weight: stride %d, dilation %d, K %d must be >= 1", stride,
          dilation, K);
  VQA_ARG(T_out == (T_in + stride - 1) / stride, "conv1d_bwd_data_weight: T_out %d != ceil(T_in/stride)", T_out);
  VQA_ARG(dy && w && x && dx && dw, "conv1d_bwd_data_weight: null tensor pointer");
  VQA_ARG(dtype == VQA_F32 || dtype == VQA_BF16, "unknown dtype %d", dtype);
  const hipStream_t s = (hipStream_t)stream;
  int pvx = 0;
  const int route = fused_route(B, T_in, T_out, C_in, C_out, K, stride, dilation, pad_left, flags, dtype, &pvx);
  if (route == F_CO1) {
    const size_t need = co1_bwd_workspace(C_in, K);
    VQA_ARG(workspace && ws_bytes >= need, "workspace too small: need %zu bytes, got %zu", need, ws_bytes);
    VQA_ARG(!(flags & VQA_ADD_RESIDUAL) || residual, "VQA_ADD_RESIDUAL without residual");
    int nparts = 0;
    const int rc = co1_bwd(dy, w, x, residual, dx, B, T_in, C_in, K, dilation, pad_left,
                           flags & (VQA_PRE_RELU | VQA_ADD_RESIDUAL | VQA_X_F32 | VQA_Y_F32), dtype, workspace,
                           &nparts, s);
    if (rc != VQA_OK) return rc;
    const int KCO = K * C_in, E = KCO + 1;
    if (desc) {
      *desc = vqa_partials_desc{(const float*)workspace, dw, db, nparts, E, KCO, 0};
      return VQA_OK;
    }
    return reduce_partials((const float*)workspace, nparts, E, KCO, dw, db, s);
  }
  if (route == F_CONV32) {
    GatherArgs a = fused_bwd_args(dy, w, x, residual, dx, B, T_in, T_out, C_in, C_out, K, dilation, pad_left, flags);
    const size_t need = fused_bwd_ws(C_in, C_out, K);
    VQA_ARG(workspace && ws_bytes >= need, "workspace too small: need %zu bytes, got %zu", need, ws_bytes);
    a.wpart = (float*)workspace;
    int nwg = 0;
    const int rc = launch_conv32_fused(a, pvx, dtype, s, &nwg);
    if (rc != VQA_OK) return rc;
    const int KCO = K * C_in * C_out, E = KCO + C_out;
    if (desc) {
      *desc = vqa_partials_desc{(const float*)workspace, dw, db, nwg, E, KCO, 0};
      return VQA_OK;
    }
    return reduce_partials((const float*)workspace, nwg, E, KCO, dw, db, s);
  }
  // not fusable here: data gradient, then the weight gradient from the same operands. A weight gradient the
  // library cannot serve is refused before the data gradient is launched.
  WgradPlan wp{};
  int rc = wgrad_route(&wp, dtype, B, T_in, T_out, C_in, C_out, K, stride, dilation, conv_wgrad_flags(flags));
  if (rc != VQA_OK) return rc;
  const bool relu = flags & VQA_PRE_RELU;
  rc = vqa_conv1d_bwd_data(dy, w, relu ? x : nullptr, residual, dx, B, T_in, T_out, C_in, C_out, K, stride, dilation,
                           pad_left, two_call_data_flags(flags), dtype, stream);
  if (rc != VQA_OK) return rc;
  return run_wgrad(x, dy, dw, db, B, T_in, T_out, C_in, C_out, K, stride, dilation, pad_left,
                   conv_wgrad_flags(flags), dtype, workspace, ws_bytes, s, desc);
}

// ---- which kernel a conv call runs (host only)
static void gather_detail(const GatherArgs& a, int dtype, int* family, int* d) {
  const GatherRoute r = gather_route(a, dtype);
  switch (r.family) {
    case G_CONV32:
      *family = VQA_ROUTE_CONV32;
      d[0] = a.O, d[1] = r.pvx, d[2] = gather_nep(a, false), d[3] = 0;
      break;
    case G_MFMA:
      *family = VQA_ROUTE_GATHER_MFMA;
      d[0] = a.C, d[1] = a.O, d[2] = r.m.pv, d[3] = r.m.tm, d[4] = r.m.nep;
      break;
    case G_CI1: *family = VQA_ROUTE_CI1, d[0] = a.O, d[1] = a.K == 4 ? 4 : 0; break;
    case G_THINO: *family = VQA_ROUTE_THIN_O, d[0] = a.C; break;
    case G_THIN: *family = VQA_ROUTE_THIN, d[0] = a.O % 8 == 0 ? 8 : 1; break;
    default: *family = VQA_ROUTE_DIRECT; d[0] = a.C, d[1] = a.O; break;
  }
}

static int gather_route_rc(const GatherArgs& a, int dtype, int* family, int* d) {
  const int rc = gather_check(a, dtype);
  if (rc != VQA_OK) return rc;
  gather_detail(a, dtype, family, d);
  VQA_REQUIRE(*family != VQA_ROUTE_THIN || gather_thin_fits(a), VQA_E_UNSUPPORTED, "thin conv: tensor too large");
  return VQA_OK;
}

static int wgrad_route_rc(int dtype, int B, int T_in, int T_out, int C, int O, int K, int S, int D, int flags,
                          int* family, int* d) {
  WgradPlan p{};
  const int rc = wgrad_route(&p, dtype, B, T_in, T_out, C, O, K, S, D, flags);
  if (rc != VQA_OK) return rc;
  *family = p.kind == WG_MFMA ? VQA_ROUTE_WGRAD_MFMA : (p.kind == WG_DIRECT ? VQA_ROUTE_WGRAD_DIRECT : VQA_ROUTE_WGRAD_THIN);
  d[0] = C, d[1] = O, d[2] = p.TT;
  if (p.kind == WG_THIN_X || p.kind == WG_THIN_G) d[2] = p.kind == WG_THIN_X ? 1 : 0;
  return VQA_OK;
}

extern "C" int vqa_conv1d_route(int op, int B, int T_in, int T_out, int C_in, int C_out, int K, int stride,
                                int dilation, int pad_left, int flags, int dtype, int* detail) {
  int d[VQA_ROUTE_DETAIL] = {0}, family = -1, rc = VQA_OK;
  VQA_ARG(dtype == VQA_F32 || dtype == VQA_BF16, "unknown dtype %d", dtype);
  VQA_ARG(stride >= 1 && dilation >= 1 && K >= 1, "conv1d_route: stride %d, dilation %d, K %d must be >= 1", stride,
          dilation, K);
  const bool transposed = op == VQA_OP_T_FWD || op == VQA_OP_T_BWD_DATA || op == VQA_OP_T_BWD_WEIGHT;
  if (transposed) {
    if ((rc = convT_check(K, stride, pad_left))) return rc;
    VQA_ARG(T_out == stride * T_in, "conv1d_route: T_out %d != stride*T_in", T_out);
  } else {
    VQA_ARG(T_out == (T_in + stride - 1) / stride, "conv1d_route: T_out %d != ceil(T_in/stride)", T_out);
  }
  const bool co1 = !transposed && co1_supported(C_in, C_out, K, stride, dilation, dtype, flags);
  switch (op) {
    case VQA_OP_FWD:
      if (co1) {
        family = VQA_ROUTE_CO1, d[0] = C_in;
      } else {
        rc = gather_route_rc(conv_fwd_gather(nullptr, nullptr, nullptr, nullptr, nullptr, B, T_in, T_out, C_in, C_out,
                                             K, stride, dilation, pad_left, flags),
                             dtype, &family, d);
      }
      break;
    case VQA_OP_BWD_DATA:
      if (co1) {
        family = VQA_ROUTE_CO1, d[0] = C_in;
      } else {
        GatherArgs a{};
        rc = conv_bwd_data_gather(&a, nullptr, nullptr, nullptr, nullptr, nullptr, B, T_in, T_out, C_in, C_out, K,
                                  stride, dilation, pad_left, flags);
        if (rc == VQA_OK) rc = gather_route_rc(a, dtype, &family, d);
      }
      break;
    case VQA_OP_BWD_WEIGHT:
      rc = wgrad_route_rc(dtype, B, T_in, T_out, C_in, C_out, K, stride, dilation, conv_wgrad_flags(flags),
                          &family, d);
      break;
    case VQA_OP_BWD_DATA_WEIGHT: {
      VQA_ARG(B > 0 && T_in > 0 && C_in > 0 && C_out > 0, "non-positive shape");
      int pvx = 0;
      const int route = fused_route(B, T_in, T_out, C_in, C_out, K, stride, dilation, pad_left, flags, dtype, &pvx);
      if (route == F_CO1) {
        family = VQA_ROUTE_CO1, d[0] = C_in;
      } else if (route == F_CONV32) {
        const GatherArgs a = fused_bwd_args(nullptr, nullptr, nullptr, nullptr, nullptr, B, T_in, T_out, C_in, C_out,
                                            K, dilation, pad_left, flags);
        family = VQA_ROUTE_CONV32;
        d[0] = a.O, d[1] = pvx, d[2] = gather_nep(a, true), d[3] = 1;
      } else {
        // detail: the families of the two calls; their own details come from a query of each op
        int scratch[VQA_ROUTE_DETAIL] = {0};
        rc = wgrad_route_rc(dtype, B, T_in, T_out, C_in, C_out, K, stride, dilation, conv_wgrad_flags(flags), &d[1],
                            scratch);
        if (rc != VQA_OK) return rc;
        const int data = vqa_conv1d_route(VQA_OP_BWD_DATA, B, T_in, T_out, C_in, C_out, K, stride, dilation, pad_left,
                                          two_call_data_flags(flags), dtype, scratch);
        if (data < 0) return data;
        d[0] = data;
        family = VQA_ROUTE_TWO_CALL;
      }
      break;
    }
    case VQA_OP_T_FWD:
      rc = gather_route_rc(convT_fwd_gather(nullptr, nullptr, nullptr, nullptr, nullptr, B, T_in, T_out, C_in, C_out, K,
                                            pad_left, flags),
                           dtype, &family, d);
      break;
    case VQA_OP_T_BWD_DATA:
      rc = gather_route_rc(convT_bwd_data_gather(nullptr, nullptr, nullptr, nullptr, nullptr, B, T_in, T_out, C_in,
                                                 C_out, K, stride, pad_left, flags),
                           dtype, &family, d);
      break;
    case VQA_OP_T_BWD_WEIGHT:
      rc = wgrad_route_rc(dtype, B, T_out, T_in, C_out, C_in, K, stride, 1, convT_wgrad_flags(flags), &family, d);
      break;
    default: vqa::set_error("conv1d_route: unknown op %d", op); return VQA_E_INVALID_ARG;
  }
  if (rc != VQA_OK) return rc;
  if (detail)
    for (int i = 0; i < VQA_ROUTE_DETAIL; ++i) detail[i] = d[i];
  return family;
}
