// vqa_spectral_stockham.hip — the spectral loss's frame-pair kernel in Stockham form (n_fft = 256, 512, 1024).
//
// ONE WAVE PER FRAME PAIR (no workgroup barrier after the table load): each wave owns an LDS buffer of N
// complex values and runs the Stockham FFT in it with register-resident radix-16 / 8 / 4 / 2 butterflies
// (2048 = 16.16.8, 1024 = 16.16.4, 512 = 8.8.8, 256 = 16.16: three passes instead of the four to six of a
// radix-8 / radix-4 plan). A pass loads every input of the lane's butterflies before it stores an output, and
// all lanes of a wave execute each LDS instruction together (in order), so the passes run IN PLACE in one
// buffer with no barrier between them. The first forward pass reads the windowed samples straight from HBM
// (lane j of butterfly j takes samples j + r N/R: coalesced), the last inverse pass writes the windowed frame
// gradients straight to HBM (samples q + S k: coalesced); the next pair's samples and target magnitudes are
// prefetched into registers while the current pair is transformed.
#include "vqa_spectral.h"
#include <algorithm>

namespace vqa {

// the radix plan of an N-point FFT: radix of pass s (0 when there is no such pass)
template <int N, int P> constexpr int wradix() {
  if constexpr (N == 2048) return P < 2 ? 16 : (P == 2 ? 8 : 0);
  else if constexpr (N == 1024) return P < 2 ? 16 : (P == 2 ? 4 : 0);
  else if constexpr (N == 512) return P < 3 ? 8 : 0;
  else return P < 2 ? 16 : 0;  // 256
}
template <int N, int P> constexpr int wstride() { return P == 0 ? 1 : wstride<N, (P > 0 ? P - 1 : 0)>() * wradix<N, (P > 0 ? P - 1 : 0)>(); }

constexpr int kSpecWaves = 4;  // waves (frame pairs in flight) per workgroup

// the pass twiddles W_N^{k e}, k < R (conjugated for the inverse), from the fp64-rounded table; VQA_SPEC_TWD:
// only k = 1, 2, 4, 8 from the table, the others one complex product away (fewer LDS reads, +1 ulp)
template <int R, bool INV> __device__ __forceinline__ void pass_twiddles(f32x2 (&w)[R], const f32x2* tw, int e) {
  w[0] = f32x2{1.f, 0.f};
#ifdef VQA_SPEC_TWD
#pragma unroll
  for (int k = 1; k < R; k <<= 1) w[k] = tw[k * e];
#pragma unroll
  for (int k = 3; k < R; ++k)
    if (k & (k - 1)) w[k] = cmul(w[k & -k], w[k - (k & -k)]);
#else
#pragma unroll
  for (int k = 1; k < R; ++k) w[k] = tw[k * e];
#endif
  if (INV) {
#pragma unroll
    for (int k = 1; k < R; ++k) w[k] = conj2(w[k]);
  }
}

// one Stockham pass of radix R at stride S over the wave's buffer z (in place): butterfly j = q + S p reads
// z[q + S (p + r m)] and writes z[q + S (R p + k)] = W_N^{k p S} DFT_R(...)_k. Every load of the lane precedes
// its first store (all lanes of the wave execute each LDS instruction together).
template <int N, int R, int S, bool INV>
__device__ __forceinline__ void wpass(f32x2* z, const f32x2* tw, int lane) {
  constexpr int m = N / (S * R), NBF = N / R, IT = (NBF + 63) / 64;
  f32x2 v[IT][R];
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int j = lane + 64 * it;
    if (NBF % 64 == 0 || j < NBF) {
      const int p = j / S, q = j - p * S;
#pragma unroll
      for (int r = 0; r < R; ++r) v[it][r] = z[pidx(q + S * (p + r * m))];
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int j = lane + 64 * it;
    if (NBF % 64 == 0 || j < NBF) {
      const int p = j / S, q = j - p * S;
      dft<R, INV>(v[it]);
      if constexpr (m == 1) {
        // the last pass (p = 0): every twiddle is W^0
#pragma unroll
        for (int k = 0; k < R; ++k) z[pidx(q + S * k)] = v[it][k];
      } else {
        f32x2 w[R];
        pass_twiddles<R, INV>(w, tw, p * S);
#pragma unroll
        for (int k = 0; k < R; ++k) z[pidx(q + S * (R * p + k))] = k ? cmul(v[it][k], w[k]) : v[it][k];
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// the target-magnitude launches (PAIR_MAG, no gradient half) at 5 / 3 waves per SIMD for N = 512 / 1024: their few
// spilled registers cost less than the third round of pairs they save (512: 25.1 -> 21.6 us, 1024: 29.3 -> 26.5 us;
// the gradient launches spill inside their passes at that occupancy and took twice as long, so they keep theirs;
// profiles/r6_spectral_occ.txt). PAIR_MAG_SELF takes the hint of PAIR_MAG.
template <int N, int MODE> constexpr int spec_pair_min_waves() {
  return MODE == PAIR_MAG || MODE == PAIR_MAG_SELF ? (N == 512 ? 5 : (N == 1024 ? 3 : 1)) : 1;
}
template <int N, int MODE>
__global__ __launch_bounds__(64 * kSpecWaves) __attribute__((amdgpu_waves_per_eu(spec_pair_min_waves<N, MODE>(), 8)))
void spec_pair_kernel(SpecPairArgs a) {
  constexpr bool GRAD = MODE == PAIR_GRAD, SELF = MODE == PAIR_MAG_SELF, MAG = MODE == PAIR_MAG || SELF;
  constexpr int KB = N / 2 + 1, NB = (KB + 63) / 64;
  constexpr int R0 = wradix<N, 0>(), R1 = wradix<N, 1>(), R2 = wradix<N, 2>();
  constexpr int S1 = wstride<N, 1>(), S2 = wstride<N, 2>();
  constexpr int NBF0 = N / R0, IT0 = (NBF0 + 63) / 64, M0 = N / R0;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  f32x2* tw = (f32x2*)smem;
  float* wn = (float*)(tw + N);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  f32x2* z = (f32x2*)(wn + N) + (size_t)wave * fpad<N>();

  // twiddles, and the window zero-padded to N (the FFT's zero padding without a per-sample branch)
  if constexpr (SELF) {
    for (int e = threadIdx.x; e < N; e += 64 * kSpecWaves) {
      tw[e] = spec_twiddle(e, N);
      wn[e] = e < a.win ? spec_hann(e, a.win) : 0.f;
    }
  } else {
    for (int e = threadIdx.x; e < N / 2; e += 64 * kSpecWaves) ((float4*)tw)[e] = ((const float4*)a.tw)[e];
    for (int e = threadIdx.x; e < N; e += 64 * kSpecWaves) wn[e] = e < a.win ? a.wn[e] : 0.f;
  }
  __syncthreads();

  const int nframes = a.B * a.F, npairs = (nframes + 1) / 2;
  const int gw = blockIdx.x * kSpecWaves + wave, nw = gridDim.x * kSpecWaves;
  // the pair's raw samples in pass-0 order (butterfly j = lane + 64 it, input r: sample j + r M0), loaded one
  // pair ahead; its target magnitudes (bin lane + 64 j) are requested when the pair starts and land during its
  // forward passes
  float ra[IT0][R0], rb[IT0][R0], ta[MAG ? 1 : NB], tb[MAG ? 1 : NB];
  auto frame_base = [&](int f) {
    const int bb_ = f / a.F;
    return a.r + (size_t)bb_ * a.T + (size_t)(f - bb_ * a.F) * a.hop;
  };
  auto load_samples = [&](int pp) {
    const float* sa = frame_base(min(2 * pp, nframes - 1));
    const float* sb = frame_base(min(2 * pp + 1, nframes - 1));
#pragma unroll
    for (int it = 0; it < IT0; ++it)
#pragma unroll
      for (int r = 0; r < R0; ++r) {
        const int n = lane + 64 * it + r * M0, nc = n < a.win ? n : 0;
        ra[it][r] = sa[nc];
        rb[it][r] = sb[nc];
      }
  };
  if (gw < npairs) load_samples(gw);
  for (int pp = gw; pp < npairs; pp += nw) {
    const int fa = 2 * pp, fb = fa + 1;
    const bool acta = fa < nframes, actb = fb < nframes;
    if constexpr (!MAG) {
      const int pa = min(fa, nframes - 1), pb = min(fb, nframes - 1);
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int k = lane + 64 * j, kc = k < KB ? k : 0;
        ta[j] = a.tm[(size_t)pa * KB + kc];
        tb[j] = a.tm[(size_t)pb * KB + kc];
      }
    }
    // pass 0 from the registers: windowed samples (n >= win: the FFT's zero padding), one butterfly at a time
#pragma unroll
    for (int it = 0; it < IT0; ++it) {
      const int p = lane + 64 * it;  // S = 1: q = 0
      if (NBF0 % 64 == 0 || p < NBF0) {
        f32x2 v[R0];
#pragma unroll
        for (int r = 0; r < R0; ++r) {
          const float w = wn[p + r * M0];
          v[r] = f32x2{ra[it][r] * w, rb[it][r] * w};
        }
        dft<R0, false>(v);
        f32x2 w[R0];
        pass_twiddles<R0, false>(w, tw, p);
#pragma unroll
        for (int k = 0; k < R0; ++k) z[pidx(R0 * p + k)] = k ? cmul(v[k], w[k]) : v[k];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
    if (pp + nw < npairs) load_samples(pp + nw);  // lands during this pair's remaining passes
    wpass<N, R1, S1, false>(z, tw, lane);
    if constexpr (R2 > 0) wpass<N, R2, S2, false>(z, tw, lane);
    // bins: |S_a|, |S_b|, the loss partials and (GRAD) H = H_a + i H_b in place
    float sda = 0.f, sxa = 0.f, sdb = 0.f, sxb = 0.f;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int k = lane + 64 * j;
      if (k < KB) {
        // bins k and N-k are read and (GRAD) rewritten by this lane only
        const int km = (N - k) & (N - 1);
        const f32x2 zk = z[pidx(k)], zm = z[pidx(km)];
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
            // G/2 (G at k = 0, N/2)
            // 1/|R| by v_rcp_f32 (1 ulp): the gradient's tolerance is 1e-4 of its max, the loss does not use it
            const float ga = mra > 0.f ? (mra - ta[j]) * __builtin_amdgcn_rcpf(mra) : 0.f;
            const float gb = mrb > 0.f ? (mrb - tb[j]) * __builtin_amdgcn_rcpf(mrb) : 0.f;
            const f32x2 Ga = f32x2{ga * rka.x, ga * rka.y}, Gb = f32x2{gb * rkb.x, gb * rkb.y};
            if (k == 0 || k == N / 2) {
              z[pidx(k)] = f32x2{Ga.x, Gb.x};
            } else {
              z[pidx(k)] = f32x2{0.5f * Ga.x - 0.5f * Gb.y, 0.5f * Ga.y + 0.5f * Gb.x};
              z[pidx(km)] = f32x2{0.5f * Ga.x + 0.5f * Gb.y, 0.5f * Gb.x - 0.5f * Ga.y};
            }
          }
        }
      }
    }
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
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
      // inverse FFT: passes 0 .. P-2 in LDS, the last pass straight to the frame gradients (windowed)
      constexpr int RL = R2 > 0 ? R2 : R1, SL = R2 > 0 ? S2 : S1, NBFL = N / RL, ITL = (NBFL + 63) / 64;
      wpass<N, R0, 1, true>(z, tw, lane);
      if constexpr (R2 > 0) wpass<N, R1, S1, true>(z, tw, lane);
      f32x2 v[ITL][RL];
#pragma unroll
      for (int it = 0; it < ITL; ++it) {
        const int q = lane + 64 * it;  // the last pass: m = 1, p = 0, butterfly j = q < S
        if (NBFL % 64 == 0 || q < NBFL) {
#pragma unroll
          for (int r = 0; r < RL; ++r) v[it][r] = z[pidx(q + SL * r)];
        }
      }
      float* oa = a.out + (size_t)fa * a.win;
      float* ob = a.out + (size_t)fb * a.win;
#pragma unroll
      for (int it = 0; it < ITL; ++it) {
        const int q = lane + 64 * it;
        if (NBFL % 64 == 0 || q < NBFL) {
          dft<RL, true>(v[it]);
#pragma unroll
          for (int k = 0; k < RL; ++k) {
            const int n = q + SL * k;
            if (n < a.win) {
              if (acta) oa[n] = v[it][k].x * wn[n];
              if (actb) ob[n] = v[it][k].y * wn[n];
            }
          }
        }
      }
    }
    // the next pair's pass 0 rewrites z: every read of it above precedes those stores in the wave's order
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  }
}

template <int N, int MODE>
static int launch_pairs(const SpecPairArgs& pa, hipStream_t s) {
  constexpr int FPI = kSpecWaves;  // frame pairs (one per wave) in flight per workgroup
  const size_t lds = (size_t)N * sizeof(f32x2) + (size_t)N * sizeof(float) + (size_t)FPI * fpad<N>() * sizeof(f32x2);
  const void* fn = (const void*)spec_pair_kernel<N, MODE>;
  if (int rc = raise_dyn_lds(fn, lds, "spec_pair_kernel")) return rc;
  // persistent: as many workgroups as fit on the chip at once (LDS-bound), each wave walking its pairs with the
  // next pair's samples prefetched; the tables are loaded once per workgroup
  const int npairs = (pa.B * pa.F + 1) / 2;
  const int groups = (npairs + FPI - 1) / FPI;
  const int grid = std::min(groups, cu_count() * resident_per_cu(fn, 64 * kSpecWaves, lds));
  hipLaunchKernelGGL((spec_pair_kernel<N, MODE>), dim3(grid), dim3(64 * kSpecWaves), lds, s, pa);
  VQA_LAUNCHED("spec_pair_kernel");
  return VQA_OK;
}

template <int MODE>
static int pairs_by_size(int n_fft, const SpecPairArgs& pa, hipStream_t s) {
  switch (n_fft) {
    case 256: return launch_pairs<256, MODE>(pa, s);
    case 512: return launch_pairs<512, MODE>(pa, s);
    case 1024: return launch_pairs<1024, MODE>(pa, s);
    default: set_error("spectral: Stockham pair kernel: n_fft %d not built", n_fft); return VQA_E_UNSUPPORTED;
  }
}

int spec_pairs_stockham(int mode, int n_fft, const SpecPairArgs& pa, hipStream_t s) {
  switch (mode) {
    case PAIR_LOSS: return pairs_by_size<PAIR_LOSS>(n_fft, pa, s);
    case PAIR_GRAD: return pairs_by_size<PAIR_GRAD>(n_fft, pa, s);
    case PAIR_MAG: return pairs_by_size<PAIR_MAG>(n_fft, pa, s);
    case PAIR_MAG_SELF: return pairs_by_size<PAIR_MAG_SELF>(n_fft, pa, s);
    default: set_error("spectral: pair mode %d unknown", mode); return VQA_E_INVALID_ARG;
  }
}

}  // namespace vqa
