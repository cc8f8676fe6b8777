// vqa_spectral.h — what the two FFT engines of the spectral loss (vqa_spectral_stockham.hip,
// vqa_spectral_fourstep.hip) and its entries (vqa_spectral.hip) share: complex helpers, the padded LDS index, the
// register butterflies, the pair kernels' arguments and modes, the table formulas, and one host dispatch function per
// engine.
#pragma once
#include "vqa_launch.h"

namespace vqa {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// complex product with fused multiply-adds (4 VALU instead of 6; one rounding less per component)
__device__ __forceinline__ f32x2 cmul(f32x2 a, f32x2 b) {
  return f32x2{__builtin_fmaf(a.x, b.x, -(a.y * b.y)), __builtin_fmaf(a.x, b.y, a.y * b.x)};
}
__device__ __forceinline__ f32x2 conj2(f32x2 a) { return f32x2{a.x, -a.y}; }
// |z| by the hardware square root (v_sqrt_f32, 1 ulp): the correctly rounded sqrtf expands to a scaling sequence
// (class test, selects, two multiplies) per value
__device__ __forceinline__ float cabs_hw(f32x2 a) { return __builtin_amdgcn_sqrtf(a.x * a.x + a.y * a.y); }

// LDS buffers of N complex values are PADDED: element i lives at pidx(i) = i + i/8, which makes the stride-8 writes of
// a first radix-8 pass (and the 64-element jumps of the second) bank-conflict-free
__device__ __forceinline__ int pidx(int i) { return i + (i >> 3); }
template <int N> constexpr int fpad() { return N + N / 8; }  // padded buffer length (elements)

constexpr int SPEC_MAX_RES = 8;

// The tables of one resolution, evaluated in fp64 and rounded once: the twiddle W_N^k = exp(-2 pi i k / N) and the
// periodic Hann window (tf.signal.hann_window(win, periodic=True)). spec_tables_kernel stores them for the training
// launches; the PAIR_MAG_SELF prologues evaluate them in place.
__device__ __forceinline__ f32x2 spec_twiddle(int k, int N) {
  double sn, cs;
  sincospi(2.0 * (double)k / (double)N, &sn, &cs);
  return f32x2{(float)cs, (float)-sn};
}
__device__ __forceinline__ float spec_hann(int n, int win) {
  return (float)(0.5 - 0.5 * cospi(2.0 * (double)n / (double)win));
}

// Frames in PAIRS (a, b): ONE complex FFT of z = w*s_a + i w*s_b gives both real frames' spectra
// (S_a[k] = (Z[k] + conj Z[N-k]) / 2, S_b[k] = (Z[k] - conj Z[N-k]) / 2i). MAG writes |S| (the target's
// spectrograms, once per step); LOSS / GRAD compare |S| of the reconstruction against the precomputed
// target magnitudes and GRAD runs ONE inverse FFT of H_a + i H_b (both adjoint outputs are real, so
// y_a = Re, y_b = Im). One FFT per frame (two with the gradient) instead of the three of a direct form.
// MAG_SELF is MAG with the tables evaluated in the kernel's prologue instead of copied from tw / wn
// (vqa_stft_magnitude, which has no workspace to keep tables in): the same values, so the same magnitudes to the bit.
enum { PAIR_LOSS = 0, PAIR_GRAD = 1, PAIR_MAG = 2, PAIR_MAG_SELF = 3 };
struct SpecPairArgs {
  const float* r;   // signal (B, T) fp32: reconstruction (LOSS, GRAD) or target (MAG, MAG_SELF)
  const float* tm;  // LOSS / GRAD: target magnitudes (B*F, N/2+1)
  float* out;       // GRAD: unscaled frame gradients (B*F, win); MAG, MAG_SELF: magnitudes (B*F, N/2+1)
  float* part;      // LOSS / GRAD: per-frame (sum (|X|-|R|)^2, sum |X|^2)
  const float* tw;  // N twiddles (re, im); null for MAG_SELF
  const float* wn;  // window; null for MAG_SELF
  int B, T, F, hop, win;
};

// the pair kernels of one engine for a PAIR_* mode and an n_fft that engine serves (dispatch_pairs, vqa_spectral.hip)
int spec_pairs_stockham(int mode, int n_fft, const SpecPairArgs& pa, hipStream_t s);  // 256, 512, 1024
int spec_pairs_fourstep(int mode, int n_fft, const SpecPairArgs& pa, hipStream_t s);  // 2048

// cos / sin (2 pi e / 16), e = 0..15 (the radix-16 butterfly's internal twiddles)
__device__ constexpr float kC16[16] = {1.f, 0.92387953251128676f, 0.70710678118654752f, 0.38268343236508977f, 0.f,
                                       -0.38268343236508977f, -0.70710678118654752f, -0.92387953251128676f, -1.f,
                                       -0.92387953251128676f, -0.70710678118654752f, -0.38268343236508977f, 0.f,
                                       0.38268343236508977f, 0.70710678118654752f, 0.92387953251128676f};
template <int E, bool INV> __device__ __forceinline__ f32x2 w16mul(f32x2 a) {
  constexpr int e = E & 15;
  if constexpr (e == 0) return a;
  else if constexpr (e == 4) return INV ? f32x2{-a.y, a.x} : f32x2{a.y, -a.x};  // +-i
  else if constexpr (e == 8) return f32x2{-a.x, -a.y};
  else if constexpr (e == 12) return INV ? f32x2{a.y, -a.x} : f32x2{-a.y, a.x};
  else {
    const float c = kC16[e], sn = kC16[(e + 12) & 15];  // sin(2 pi e/16) = cos(2 pi (e - 4)/16)
    const f32x2 w = INV ? f32x2{c, sn} : f32x2{c, -sn};
    return cmul(a, w);
  }
}

// X[k] = sum_r a[r] W_R^{rk} in place (W_R = exp(-+2 pi i / R)), natural order
template <bool INV> __device__ __forceinline__ void dft4(f32x2& a0, f32x2& a1, f32x2& a2, f32x2& a3) {
  const f32x2 b0 = a0 + a2, b1 = a0 - a2, b2 = a1 + a3, d = a1 - a3;
  const f32x2 jd = INV ? f32x2{-d.y, d.x} : f32x2{d.y, -d.x};
  a0 = b0 + b2;
  a1 = b1 + jd;
  a2 = b0 - b2;
  a3 = b1 - jd;
}
template <int R, bool INV> __device__ __forceinline__ void dft(f32x2 (&a)[R]) {
  if constexpr (R == 2) {
    const f32x2 t = a[0] - a[1];
    a[0] = a[0] + a[1];
    a[1] = t;
  } else if constexpr (R == 4) {
    dft4<INV>(a[0], a[1], a[2], a[3]);
  } else if constexpr (R == 8) {
    // r = r1 + 2 r2 (r1 < 2, r2 < 4): 4-point DFTs over r2, W8^{r1 k2}, 2-point DFTs over r1
    dft4<INV>(a[0], a[2], a[4], a[6]);
    dft4<INV>(a[1], a[3], a[5], a[7]);
    a[3] = w16mul<2, INV>(a[3]);
    a[5] = w16mul<4, INV>(a[5]);
    a[7] = w16mul<6, INV>(a[7]);
    f32x2 o[8];
#pragma unroll
    for (int k2 = 0; k2 < 4; ++k2) {
      o[k2] = a[2 * k2] + a[2 * k2 + 1];
      o[k2 + 4] = a[2 * k2] - a[2 * k2 + 1];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = o[k];
  } else if constexpr (R == 16) {
    // r = r1 + 4 r2: 4-point DFTs over r2 (B[r1][k2] lands in a[r1 + 4 k2]), W16^{r1 k2}, 4-point DFTs over r1
#pragma unroll
    for (int r1 = 0; r1 < 4; ++r1) dft4<INV>(a[r1], a[r1 + 4], a[r1 + 8], a[r1 + 12]);
    a[5] = w16mul<1, INV>(a[5]);
    a[9] = w16mul<2, INV>(a[9]);
    a[13] = w16mul<3, INV>(a[13]);
    a[6] = w16mul<2, INV>(a[6]);
    a[10] = w16mul<4, INV>(a[10]);
    a[14] = w16mul<6, INV>(a[14]);
    a[7] = w16mul<3, INV>(a[7]);
    a[11] = w16mul<6, INV>(a[11]);
    a[15] = w16mul<9, INV>(a[15]);
    f32x2 o[16];
#pragma unroll
    for (int k2 = 0; k2 < 4; ++k2) {
      f32x2 c0 = a[4 * k2], c1 = a[4 * k2 + 1], c2 = a[4 * k2 + 2], c3 = a[4 * k2 + 3];
      dft4<INV>(c0, c1, c2, c3);
      o[k2] = c0;
      o[k2 + 4] = c1;
      o[k2 + 8] = c2;
      o[k2 + 12] = c3;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) a[k] = o[k];
  }
}

}  // namespace vqa
