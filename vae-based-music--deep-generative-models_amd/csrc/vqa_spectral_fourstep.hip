// vqa_spectral_fourstep.hip — the spectral loss's frame-pair kernel as a FOUR-STEP FFT held in registers (round 6;
// built and launched for n_fft = 2048 only: dispatch_pairs in vqa_spectral.hip says why).
//
// N = P x 64, P = N / 64 = 32 points per lane, one wave per frame pair as in the Stockham form. Forward, with
// n = 64 n1 + n2, k = k1 + P k2:
//   lane n2 loads z[64 n1 + n2] (n1 < P), P-point DFT over n1 in registers, times W_N^{n2 k1}
//   -> ONE transpose through the wave's LDS buffer: the 64-point DFT of index k1 goes to the G = 64 / P = 2 lanes
//      (k1, g), lane g holding n2 = g + G m (m < P)
//   P-point DFT over m in registers, times W_64^{g q}, then the 2-point DFT across the two lanes (one quad_perm DPP
//      exchange, no LDS) -> lane (k1, g) holds Z[k1 + P (q + P g)], q < P
//   the pair separation needs Z[N - k] beside Z[k]: ONE exchange through the LDS buffer (every lane writes its bins
//      at their natural index, reads the mirror bins)
// and the inverse (GRAD) runs the same steps backwards (cross-lane DFT, P-point DFT, W_N^{-n2 k1}, transpose,
// P-point DFT, windowed stores of the frame gradients at n = lane + 64 n1). Three passes through LDS per pair where
// the Stockham form makes five to seven, and its per-butterfly twiddle reads are replaced by one table row per
// lane (W_N^{n2 k1} laid out [k1][n2] at a padded pitch) and compile-time constants. LDS layouts (8-byte slots):
// the transpose rows have pitch 64 + G (the strided side hits 32 distinct slots per half wave) and the bin exchange
// puts bin k at k + (k / P^2) 32 / G (both the own and the mirror accesses conflict-free, tools/spec4_banks.py).
// Same loss / gradient definition and the same fp64-rounded twiddle and window tables as spec_pair_kernel.
#include "vqa_spectral.h"
#include <utility>
#include <algorithm>

namespace vqa {

__device__ constexpr float kC32[32] = {
    1.f, 0.98078528040323043f, 0.92387953251128674f, 0.83146961230254524f, 0.70710678118654757f,
    0.55557023301960229f, 0.38268343236508984f, 0.19509032201612833f, 0.f, -0.19509032201612819f,
    -0.38268343236508973f, -0.55557023301960196f, -0.70710678118654746f, -0.83146961230254535f,
    -0.92387953251128674f, -0.98078528040323043f, -1.f, -0.98078528040323043f, -0.92387953251128685f,
    -0.83146961230254546f, -0.70710678118654768f, -0.55557023301960218f, -0.38268343236509034f,
    -0.19509032201612866f, 0.f, 0.1950903220161283f, 0.38268343236509f, 0.55557023301960184f,
    0.70710678118654735f, 0.83146961230254524f, 0.92387953251128652f, 0.98078528040323032f};
template <int E, bool INV> __device__ __forceinline__ f32x2 w32mul(f32x2 a) {
  constexpr int e = E & 31;
  if constexpr ((e & 1) == 0) {
    return w16mul<e / 2, INV>(a);
  } else {
    const float c = kC32[e], sn = kC32[(e + 24) & 31];  // sin(2 pi e/32) = cos(2 pi (e - 8)/32)
    return cmul(a, INV ? f32x2{c, sn} : f32x2{c, -sn});
  }
}
template <bool INV, int... K>
__device__ __forceinline__ void dft32_combine(f32x2 (&a)[32], const f32x2 (&ev)[16], const f32x2 (&od)[16],
                                              std::integer_sequence<int, K...>) {
  ((a[K] = ev[K] + w32mul<K, INV>(od[K]), a[K + 16] = ev[K] - w32mul<K, INV>(od[K])), ...);
}
// natural-order P-point DFT in registers (P = 32: two 16-point DFTs of the even / odd inputs and one combine)
template <int P, bool INV> __device__ __forceinline__ void dftp(f32x2 (&a)[P]) {
  if constexpr (P == 32) {
    f32x2 ev[16], od[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      ev[i] = a[2 * i];
      od[i] = a[2 * i + 1];
    }
    dft<16, INV>(ev);
    dft<16, INV>(od);
    dft32_combine<INV>(a, ev, od, std::make_integer_sequence<int, 16>{});
  } else {
    dft<P, INV>(a);
  }
}
template <int N> struct Spec4 {
  static_assert(N == 2048, "the four-step kernel is written for N = 2048 (P = 32 points per lane, G = 2 lanes per k1)");
  static constexpr int P = N / 64, G = 64 / P, PITCH = 64 + G, BUF = N + 64;
  static_assert(P * PITCH <= BUF && N + 32 <= BUF, "buffer plan");
  // LDS slot of natural bin k in the exchange
  static __device__ __forceinline__ int slot(int k) { return k + (k / (P * P)) * (32 / G); }
};
// waves (frame pairs in flight) per workgroup: two per SIMD (a lone wave issues a VALU instruction every 4 cycles, two
// every 2) within 256 VGPRs, which leaves no room to prefetch the next pair's 64 sample registers: a pair's samples
// are loaded when it starts, and the other wave of the SIMD works meanwhile
constexpr int kSpec4Waves = 8;

// the 2-point DFT across the two lanes (k1, g = 0 / 1), its own inverse: the lower lane takes u + p, the upper p - u
// (p: the partner's value)
template <int P> __device__ __forceinline__ void xlane_dft(f32x2 (&c)[P], int g) {
  const bool up = (g & 1) != 0;
  const float sg = up ? -1.f : 1.f;
#pragma unroll
  for (int q = 0; q < P; ++q) {
    const f32x2 u = c[q];
    const f32x2 pv = f32x2{xl::xor1(u.x), xl::xor1(u.y)};
    c[q] = f32x2{__builtin_fmaf(sg, u.x, pv.x), __builtin_fmaf(sg, u.y, pv.y)};
  }
}

__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <int N, int MODE>
__global__ __launch_bounds__(64 * kSpec4Waves) void spec_pair4_kernel(SpecPairArgs a) {
  typedef Spec4<N> S4;
  constexpr bool GRAD = MODE == PAIR_GRAD, SELF = MODE == PAIR_MAG_SELF, MAG = MODE == PAIR_MAG || SELF;
  constexpr int W = kSpec4Waves;
  constexpr int P = S4::P, G = S4::G, PITCH = S4::PITCH, KB = N / 2 + 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  f32x2* T = (f32x2*)smem;       // T[k1 PITCH + n2] = W_N^{n2 k1}
  f32x2* tw64 = T + P * PITCH;   // W_64^e = W_N^{e P}
  float* wn = (float*)(tw64 + 64);  // window, zero-padded to N
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  f32x2* buf = (f32x2*)(wn + N) + (size_t)wave * S4::BUF;
  // W_N^e and the window from the tables of spec_tables_kernel, or (MAG_SELF) by the same formulas here
  auto twg = [&](int e) {
    if constexpr (SELF) return spec_twiddle(e, N);
    else return ((const f32x2*)a.tw)[e];
  };
  auto wng = [&](int e) {
    if constexpr (SELF) return spec_hann(e, a.win);
    else return a.wn[e];
  };
  for (int e = threadIdx.x; e < P * 64; e += 64 * W) {
    const int k1 = e >> 6, n2 = e & 63;
    T[k1 * PITCH + n2] = twg(n2 * k1);
  }
  for (int e = threadIdx.x; e < 64; e += 64 * W) tw64[e] = twg(e * P);
  for (int e = threadIdx.x; e < N; e += 64 * W) wn[e] = e < a.win ? wng(e) : 0.f;
  __syncthreads();

  const int k1s = lane / G, g = lane & (G - 1);
  const int kbase = k1s + P * P * g;  // own bin of register q: kbase + P q
  const int nframes = a.B * a.F, npairs = (nframes + 1) / 2;
  const int gw = blockIdx.x * W + wave, nw = gridDim.x * W;
  constexpr int NB = (KB + 63) / 64;
  float ra[P], rb[P], ta[MAG ? 1 : NB], tb[MAG ? 1 : NB];
  auto frame_base = [&](int f) {
    const int bb_ = f / a.F;
    return a.r + (size_t)bb_ * a.T + (size_t)(f - bb_ * a.F) * a.hop;
  };
  auto load_samples = [&](int pp) {
    const float* sa = frame_base(min(2 * pp, nframes - 1));
    const float* sb = frame_base(min(2 * pp + 1, nframes - 1));
#pragma unroll
    for (int n1 = 0; n1 < P; ++n1) {
      const int n = lane + 64 * n1, nc = n < a.win ? n : 0;
      ra[n1] = sa[nc];
      rb[n1] = sb[nc];
    }
  };
  for (int pp = gw; pp < npairs; pp += nw) {
    const int fa = 2 * pp, fb = fa + 1;
    const bool acta = fa < nframes, actb = fb < nframes;
    load_samples(pp);
    if constexpr (!MAG) {
      // target magnitudes of the lane's canonical bins lane + 64 j, requested now, used after the forward transform
      const int pa = min(fa, nframes - 1), pb = min(fb, nframes - 1);
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int k = lane + 64 * j, kc = k < KB ? k : 0;
        ta[j] = a.tm[(size_t)pa * KB + kc];
        tb[j] = a.tm[(size_t)pb * KB + kc];
      }
    }
    f32x2 c[P];
#pragma unroll
    for (int n1 = 0; n1 < P; ++n1) {
      const float w = wn[lane + 64 * n1];
      c[n1] = f32x2{ra[n1] * w, rb[n1] * w};
    }
    dftp<P, false>(c);  // over n1 -> k1
#pragma unroll
    for (int k1 = 1; k1 < P; ++k1) c[k1] = cmul(c[k1], T[k1 * PITCH + lane]);
#pragma unroll
    for (int k1 = 0; k1 < P; ++k1) buf[k1 * PITCH + lane] = c[k1];
    wave_sync_lds();
#pragma unroll
    for (int m = 0; m < P; ++m) c[m] = buf[k1s * PITCH + g + G * m];
    wave_sync_lds();
    dftp<P, false>(c);  // over m -> q
#pragma unroll
    for (int q = 1; q < P; ++q) c[q] = cmul(c[q], tw64[g * q]);  // g = 0: W^0 = 1 exactly
    xlane_dft(c, g);  // lane (k1s, g): Z[kbase + P q]
    // the bins: every lane writes its Z values at their natural slots, then takes canonical bins k = lane + 64 j
    // (k <= N / 2: each once, as spec_pair_kernel) with their mirrors N - k; GRAD writes H at k and N - k back and
    // every lane reads its own bins' H for the inverse
#pragma unroll
    for (int q = 0; q < P; ++q) buf[S4::slot(kbase + P * q)] = c[q];
    wave_sync_lds();
    float sda = 0.f, sxa = 0.f, sdb = 0.f, sxb = 0.f;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int k = lane + 64 * j;
      if (NB * 64 == KB || k < KB) {
        const int km = (N - k) & (N - 1);
        const f32x2 zk = buf[S4::slot(k)], zm = buf[S4::slot(km)];
        const f32x2 rka = f32x2{0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y)};
        const f32x2 rkb = f32x2{0.5f * (zk.y + zm.y), 0.5f * (zm.x - zk.x)};
        const float mra = cabs_hw(rka), mrb = cabs_hw(rkb);
        if constexpr (MAG) {
          if (acta) a.out[(size_t)fa * KB + k] = mra;
          if (actb) a.out[(size_t)fb * KB + k] = mrb;
        } else {
          const float da = ta[j] - mra, db = tb[j] - mrb;
          sda += da * da;
          sxa += ta[j] * ta[j];
          sdb += db * db;
          sxb += tb[j] * tb[j];
          if constexpr (GRAD) {
            // dL/d(Re,Im)R_k = (|R|-|X|) R/|R| (0 at |R| = 0); H = H_a + i H_b, each the Hermitian extension of
            // G/2 (G at k = 0, N/2) — spec_pair_kernel's values, written over Z at k and N - k at once: no later
            // iteration reads those slots (its k and N - k lie in other 64-bin bands)
            const float ga = mra > 0.f ? (mra - ta[j]) * __builtin_amdgcn_rcpf(mra) : 0.f;
            const float gb = mrb > 0.f ? (mrb - tb[j]) * __builtin_amdgcn_rcpf(mrb) : 0.f;
            const f32x2 Ga = f32x2{ga * rka.x, ga * rka.y}, Gb = f32x2{gb * rkb.x, gb * rkb.y};
            if (k == 0 || k == N / 2) {
              buf[S4::slot(k)] = f32x2{Ga.x, Gb.x};
            } else {
              buf[S4::slot(k)] = f32x2{0.5f * Ga.x - 0.5f * Gb.y, 0.5f * Ga.y + 0.5f * Gb.x};
              buf[S4::slot(km)] = f32x2{0.5f * Ga.x + 0.5f * Gb.y, 0.5f * Gb.x - 0.5f * Ga.y};
            }
          }
        }
      }
    }
    if constexpr (GRAD) {
      wave_sync_lds();
#pragma unroll
      for (int q = 0; q < P; ++q) c[q] = buf[S4::slot(kbase + P * q)];
    }
    wave_sync_lds();  // every read of buf precedes the next writes
    if constexpr (!MAG) {
      sda = warp_sum(sda);
      sxa = warp_sum(sxa);
      sdb = warp_sum(sdb);
      sxb = warp_sum(sxb);
      if (lane == 0) {
        if (acta) {
          a.part[2 * (size_t)fa] = sda;
          a.part[2 * (size_t)fa + 1] = sxa;
        }
        if (actb) {
          a.part[2 * (size_t)fb] = sdb;
          a.part[2 * (size_t)fb + 1] = sxb;
        }
      }
    }
    if constexpr (GRAD) {
      xlane_dft(c, g);  // lane (k1s, g): index g of the 64-point inverse, times W_64^{-g q}
#pragma unroll
      for (int q = 1; q < P; ++q) c[q] = cmul(c[q], conj2(tw64[g * q]));
      dftp<P, true>(c);  // over q -> m: n2 = g + G m
#pragma unroll
      for (int m = 0; m < P; ++m) {
        const int e = k1s * PITCH + g + G * m;
        c[m] = cmul(c[m], conj2(T[e]));
        buf[e] = c[m];
      }
      wave_sync_lds();
#pragma unroll
      for (int k1 = 0; k1 < P; ++k1) c[k1] = buf[k1 * PITCH + lane];
      wave_sync_lds();
      dftp<P, true>(c);  // over k1 -> n1: h[lane + 64 n1]
      float* oa = a.out + (size_t)fa * a.win;
      float* ob = a.out + (size_t)fb * a.win;
#pragma unroll
      for (int n1 = 0; n1 < P; ++n1) {
        const int n = lane + 64 * n1;
        if (n < a.win) {
          const float w = wn[n];
          if (acta) oa[n] = c[n1].x * w;
          if (actb) ob[n] = c[n1].y * w;
        }
      }
    }
  }
}

// persistent, sized by the occupancy API as the Stockham launch
template <int N, int MODE>
static int launch_pairs4(const SpecPairArgs& pa, hipStream_t s) {
  typedef Spec4<N> S4;
  const void* fn = (const void*)spec_pair4_kernel<N, MODE>;
  constexpr int W = kSpec4Waves;
  const size_t lds = (size_t)(S4::P * S4::PITCH + 64) * sizeof(f32x2) + (size_t)N * sizeof(float) +
                     (size_t)W * S4::BUF * sizeof(f32x2);
  if (int rc = raise_dyn_lds(fn, lds, "spec_pair4_kernel")) return rc;
  const int npairs = (pa.B * pa.F + 1) / 2;
  const int groups = (npairs + W - 1) / W;
  const int grid = std::min(groups, cu_count() * resident_per_cu(fn, 64 * W, lds));
  hipLaunchKernelGGL((spec_pair4_kernel<N, MODE>), dim3(grid), dim3(64 * W), lds, s, pa);
  VQA_LAUNCHED("spec_pair4_kernel");
  return VQA_OK;
}

int spec_pairs_fourstep(int mode, int n_fft, const SpecPairArgs& pa, hipStream_t s) {
  if (n_fft != 2048) {
    set_error("spectral: four-step pair kernel: n_fft %d not built", n_fft);
    return VQA_E_UNSUPPORTED;
  }
  switch (mode) {
    case PAIR_LOSS: return launch_pairs4<2048, PAIR_LOSS>(pa, s);
    case PAIR_GRAD: return launch_pairs4<2048, PAIR_GRAD>(pa, s);
    case PAIR_MAG: return launch_pairs4<2048, PAIR_MAG>(pa, s);
    case PAIR_MAG_SELF: return launch_pairs4<2048, PAIR_MAG_SELF>(pa, s);
    default: set_error("spectral: pair mode %d unknown", mode); return VQA_E_INVALID_ARG;
  }
}

}  // namespace vqa
