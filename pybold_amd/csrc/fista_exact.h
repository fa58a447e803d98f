// Register-resident fused FISTA kernel in float64 END TO END (y, scans, FIRs, iterate, cost
// trace, stop rules): the reference's own arithmetic, for the calls where its decisions
// matter to the last digit -- the 1-D calls of the API and the noise-driven lambda search,
// whose stop rule sits on a knife edge (Numerics).
//
// One problem per wave64, S consecutive samples per lane (S = 5: series of up to 320 scans;
// S = 10: 640), everything in VGPRs:
//   z = cumsum(w)          lane-local prefix + wave scan (DPP row_shr / row_bcast on both halves)
//   x = h * z              K-tap causal FIR, v_fma_f64 (full rate on gfx950); the K-1 halo
//                          samples come from the lanes below through wave_shr:1 chains
//   g = revcumsum(K^T r)   halo from the lanes above, suffix = total - inclusive prefix
//   u = w - s g ; w = u - (1+beta) clamp(u, -th, th)
// Cost trace and both stop rules as in fista_fast.h, but the window rule (wind = 6) keeps
// u_{k-1} and the last three increments in float64 REGISTERS (S is small), so its criterion
// is float64 too.  ~530 instructions per problem-iteration: a 500-iteration single-voxel
// solve takes ~0.5 ms instead of 4 ms on the LDS kernel (generic.h), a machine-filling batch
// runs at ~6x its rate.
//
// Reference: pybold/bold_signal.py:62-97 (deconv), :259-276 (_loops_deconv),
// pybold/linear.py:73-113, pybold/convolution.py:105-132.
#pragma once
#include "../../include/pybold_hip.h"
#include "common.h"
#include "fista_fast.h"
#include <type_traits>

namespace pb {

// The taps of a pass are read through a HOLDER: any type with `template <int m> double tap() const`.  TapsD keeps them
// where the by-value kernel argument puts them (scalar registers: 32 float64 taps fill the scalar file); TapsLane
// (fista_exact_long.h) keeps up to 64 of them in one VGPR pair of the wave.
template <int KT>
struct TapsD {
  double h[KT];
  template <int m>
  __host__ __device__ __forceinline__ double tap() const { return h[m]; }
};

template <int KT>
inline TapsD<KT> make_taps_d(const double* taps, int K) {
  TapsD<KT> t;
  for (int m = 0; m < KT; ++m) t.h[m] = (m < K) ? taps[m] : 0.0;
  return t;
}

template <int CTRL, int ROW_MASK = 0xf, bool BOUND = true>
__device__ __forceinline__ double dpp_f64(double v) {
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, ROW_MASK, 0xf, BOUND);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, ROW_MASK, 0xf, BOUND);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}

// inclusive prefix sum over the 64 lanes of the wave
__device__ __forceinline__ double wave_prefix_incl_f64(double t) {
  t += dpp_f64<DPP_ROW_SHR + 1>(t);
  t += dpp_f64<DPP_ROW_SHR + 2>(t);
  t += dpp_f64<DPP_ROW_SHR + 4>(t);
  t += dpp_f64<DPP_ROW_SHR + 8>(t);
  t += dpp_f64<DPP_ROW_BCAST15, 0xa, false>(t);     // rows 1, 3 += total of the row before
  t += dpp_f64<DPP_ROW_BCAST31, 0xc, false>(t);     // rows 2, 3 += total of the first half
  return t;
}

__device__ __forceinline__ double readlane_f64(double v, int lane);

// sum over the lanes ABOVE this one, built from additions only (in-row suffix scan + the totals of the rows above):
// where every lane above holds 0 the result is EXACTLY 0, as in the reference's flip-cumsum-flip
// (pybold/linear.py:43).  `total - inclusive prefix` leaves a rounding residue of ~1e-16 |total| there instead, and
// the last sample of a series has gradient exactly 0 (every SPM HRF has h[0] = 0): with a NEGATIVE threshold the
// reference's prox is discontinuous at 0 (sign(u) |th|), so that residue grew into a 1e-3 error (round 5).
__device__ __forceinline__ double wave_suffix_excl_f64(double v) {
  double s = v;
  s += dpp_f64<DPP_ROW_SHL + 1>(s);
  s += dpp_f64<DPP_ROW_SHL + 2>(s);
  s += dpp_f64<DPP_ROW_SHL + 4>(s);
  s += dpp_f64<DPP_ROW_SHL + 8>(s);                 // lane 0 of a row: the row's total
  const double t3 = readlane_f64(s, 48), t2 = readlane_f64(s, 32), t1 = readlane_f64(s, 16);
  const int row = (threadIdx.x & 63) >> 4;
  const double t23 = t2 + t3;
  const double above = row == 3 ? 0.0 : (row == 2 ? t3 : (row == 1 ? t23 : t1 + t23));
  return dpp_f64<DPP_ROW_SHL + 1>(s) + above;        // lanes above within the row (0 for the row's last lane) + rows above
}

__device__ __forceinline__ double readlane_f64(double v, int lane) {
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_readlane((int)b, lane);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}

// ---- the per-lane pieces of the pass, shared with the four-wave form (fista_exact_split.h) -------------------------------
// window of z for the FIR: own samples at [H, H+S), below them the last H samples of the lanes below (0 before lane 0)
template <int S, int KT>
__device__ __forceinline__ void exact_window_below(const double (&z)[S], double (&Z)[KT - 1 + S]) {
  constexpr int H = KT - 1;
  constexpr int D = (H + S - 1) / S;        // neighbour lanes that contribute halo
  static_assert(D <= 63, "halo spans more than the wave");
  // ---- window of z: own samples at [H, H+S), halo below -------------------
  static_for<0, S>([&](auto jc) { Z[H + decltype(jc)::value] = z[decltype(jc)::value]; });
  {
    double sh[S];
#pragma unroll
    for (int j = 0; j < S; ++j) sh[j] = z[j];
    static_for<1, D + 1>([&](auto dc) {
      constexpr int d = decltype(dc)::value;
#pragma unroll
      for (int j = 0; j < S; ++j) sh[j] = dpp_f64<DPP_WAVE_SHR1>(sh[j]);      // lane - d
      static_for<0, S>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        constexpr int e = H - d * S + j;
        if constexpr (e >= 0) Z[e] = sh[j];
      });
    });
  }
}

// window of r for the correlation: own samples at [0, S), above them the first H samples of the lanes above (0 past lane 63)
template <int S, int KT>
__device__ __forceinline__ void exact_window_above(const double (&r)[S], double (&R)[S + KT - 1]) {
  constexpr int H = KT - 1;
  constexpr int D = (H + S - 1) / S;
  // ---- window of r: own samples at [0, S), halo above ----------------------
  static_for<0, S>([&](auto jc) { R[decltype(jc)::value] = r[decltype(jc)::value]; });
  {
    double sh[S];
#pragma unroll
    for (int j = 0; j < S; ++j) sh[j] = r[j];
    static_for<1, D + 1>([&](auto dc) {
      constexpr int d = decltype(dc)::value;
#pragma unroll
      for (int j = 0; j < S; ++j) sh[j] = dpp_f64<DPP_WAVE_SHL1>(sh[j]);      // lane + d
      static_for<0, S>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        constexpr int e = d * S + j;
        if constexpr (e < S + H) R[e] = sh[j];
      });
    });
  }
}

// r = (h * z - y) on the samples of the series from the window Z of z: own samples at [H, H+S), halo below them
template <int S, int KT, class TAPS>
__device__ __forceinline__ void exact_fir_residual(const double (&Z)[KT - 1 + S], const double (&y)[S], const double (&mk)[S],
                                                   const TAPS& taps, double (&r)[S]) {
  constexpr int H = KT - 1;
  // ---- r = h * z - y -------------------------------------------------------
  static_for<0, S>([&](auto jc) { r[decltype(jc)::value] = -y[decltype(jc)::value]; });
  static_for<0, KT>([&](auto mc) {          // tap-major: S independent chains
    constexpr int m = decltype(mc)::value;
    const double hm = taps.template tap<m>();
    static_for<0, S>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      r[j] = fma(hm, Z[H + j - m], r[j]);
    });
  });
#pragma unroll
  for (int j = 0; j < S; ++j) r[j] *= mk[j];
}

// g = K^T r from the window R of r (own samples at [0, S), halo above them), summed from the lane's last sample down
template <int S, int KT, class TAPS>
__device__ __forceinline__ void exact_corr_suffix(const double (&R)[S + KT - 1], const TAPS& taps, double (&g)[S]) {
#pragma unroll
  for (int j = 0; j < S; ++j) g[j] = 0.0;
  static_for<0, KT>([&](auto mc) {
    constexpr int m = decltype(mc)::value;
    const double hm = taps.template tap<m>();
    static_for<0, S>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      g[j] = fma(hm, R[j + m], g[j]);
    });
  });
#pragma unroll
  for (int j = S - 2; j >= 0; --j) g[j] += g[j + 1];
}

// gradient step, prox, momentum on the lane's samples; with a stop rule the LANE's share of the two sums of its criterion
// comes back in num / den (and the window state moves on one iteration)
template <int S, int STOP>
__device__ __forceinline__ void exact_update(const double (&g)[S], double (&w)[S], double nstep, double th, const double* beta_k,
                                             double (&uprev)[STOP == 2 ? S : 1], double (&d1)[STOP == 2 ? S : 1],
                                             double (&d2)[STOP == 2 ? S : 1], double (&d3)[STOP == 2 ? S : 1], double& num,
                                             double& den) {
  // ---- gradient step, prox, momentum; stop rules ------------------------------
  const double beta = *beta_k;                // (read here, after the scans: the taps fill the scalar registers)
  const double nb1 = -(1.0 + beta);
  if constexpr (STOP == 0) {
#pragma unroll
    for (int j = 0; j < S; ++j) {
      const double u = fma(nstep, g[j], w[j]);
      const double d = prox_excess_ref(u, th);
      w[j] = fma(nb1, d, u);
    }
  } else {
    num = 0.0;
    den = 0.0;
#pragma unroll
    for (int j = 0; j < S; ++j) {
      const double u = fma(nstep, g[j], w[j]);
      const double d = prox_excess_ref(u, th);
      const double wn = fma(nb1, d, u);
      if constexpr (STOP == 1) {            // _loops_deconv rule (pybold/bold_signal.py:267-273)
        const double diff = wn - u;
        num = fma(diff, diff, num);
        den = fma(wn, wn, den);
      } else {
        // deconv window rule, wind = 6 (:82-95), on [u_{k-4} .. u_k, w_{k+1}]:
        //   3 (new - old) = delta_{k-3} + 2 delta_{k-2} + 3 delta_{k-1} + 2 delta_k + e
        //   3 new         = 3 u_k - delta_k + e          (see fista_fast.h)
        const double dk = u - uprev[j];
        const double e = wn - u;
        const double diff = fma(2.0, dk, fma(3.0, d1[j], fma(2.0, d2[j], d3[j]))) + e;
        const double sn = fma(3.0, u, e - dk);
        num = fma(diff, diff, num);
        den = fma(sn, sn, den);
        d3[j] = d2[j];
        d2[j] = d1[j];
        d1[j] = dk;
        uprev[j] = u;
      }
      w[j] = wn;
    }
  }
}

// ---- the pass body, shared by fista_exact_kernel and auto_lbda_kernel (fista_auto.h) --------------------------------
// Both kernels keep y, w, the mask and the window-rule state in VGPRs and call the two halves below, once per pass;
// the cost trace of fista_exact_kernel and the residual statistics of auto_lbda_kernel sit between them (or after the
// first alone), on the residual the forward half returns.

// forward half: z = cumsum(w), x = h * z, r = (x - y) on the samples of the series (0 on the padding)
template <int S, int KT, class TAPS>
__device__ __forceinline__ void exact_forward(const double (&w)[S], const double (&y)[S], const double (&mk)[S],
                                              const TAPS& taps, double (&r)[S]) {
  constexpr int H = KT - 1;
  // ---- z = cumsum(w) ----------------------------------------------------
  double z[S];
  z[0] = w[0];
#pragma unroll
  for (int j = 1; j < S; ++j) z[j] = z[j - 1] + w[j];
  {
    const double off = dpp_f64<DPP_WAVE_SHR1>(wave_prefix_incl_f64(z[S - 1]));
#pragma unroll
    for (int j = 0; j < S; ++j) z[j] += off;
  }
  double Z[H + S];
  exact_window_below<S, KT>(z, Z);
  exact_fir_residual<S, KT>(Z, y, mk, taps, r);
}

// backward half: g = revcumsum(K^T r), gradient step, prox, momentum; with a stop rule (STOP 1: _loops_deconv, 2: window,
// wind = 6) the two wave-wide sums of its criterion come back in num / den (and the window state moves on one iteration)
template <int S, int KT, int STOP, class TAPS>
__device__ __forceinline__ void exact_backward(const double (&r)[S], double (&w)[S], const TAPS& taps, double nstep,
                                               double th, const double* beta_k, double (&uprev)[STOP == 2 ? S : 1],
                                               double (&d1)[STOP == 2 ? S : 1], double (&d2)[STOP == 2 ? S : 1],
                                               double (&d3)[STOP == 2 ? S : 1], double& num, double& den) {
  constexpr int H = KT - 1;
  double R[S + H];
  exact_window_above<S, KT>(r, R);
  // ---- g = revcumsum(K^T r) ---------------------------------------------------
  double g[S];
  exact_corr_suffix<S, KT>(R, taps, g);
  {
    const double off = wave_suffix_excl_f64(g[0]);         // sum of the lanes above, exactly 0 above the last sample
#pragma unroll
    for (int j = 0; j < S; ++j) g[j] += off;
  }

  exact_update<S, STOP>(g, w, nstep, th, beta_k, uprev, d1, d2, d3, num, den);
  if constexpr (STOP != 0) {
    num = seg_allsum_f64<64>(num);
    den = seg_allsum_f64<64>(den);
  }
}

// the criterion of either stop rule on those sums: first test after 3 (_loops_deconv) / wind + 1 = 7 (window rule)
// iterations, floor 1e-10 / 3e-10 (the window rule's sums carry a factor 3)
template <int STOP>
__device__ __forceinline__ bool exact_stop_fires(int it, double num, double den, double tol) {
  constexpr int first_test = (STOP == 1) ? 3 : 6 + 1;
  constexpr double floor_eps = (STOP == 2) ? 3.0e-10 : 1.0e-10;
  return it >= first_test && sqrt(num) / (sqrt(den) + floor_eps) < tol;
}

template <int S, int KT, bool WITH_J, int STOP>
__global__ __launch_bounds__(256) void fista_exact_kernel(FistaArgs a, TapsD<KT> taps) {
  const int lane = threadIdx.x & 63;
  // slots of this launch's list (fista_fast.h: launch_slots; the batch itself without a device-side list).  Round 5: the
  // ill-conditioned series of a partitioned float32 call run here (y float32 in HBM, a.y64 == nullptr; cost trace to a.J)
  int s0, s1;
  launch_slots(a, s0, s1);
  const int slot = (int)((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) + s0;
  if (slot >= s1 && a.range) return;               // (one problem per wave: uniform; an empty candidate launch leaves here)
  bool live;
  const int p = slot_to_problem(a, slot, s1, live);
  const int base = lane * S;

  double y[S], w[S], mk[S];
  {
    const double* yrow = a.y64 ? a.y64 + (int64_t)(p / a.y_rep) * a.ldy : nullptr;
    const float* yrow32 = a.y64 ? nullptr : a.y + (int64_t)(p / a.y_rep) * a.ldy;
    const double* wrow = a.w + (int64_t)p * a.ldw;
#pragma unroll
    for (int j = 0; j < S; ++j) {
      const bool ok = base + j < a.N;
      y[j] = ok ? (yrow ? yrow[base + j] : (double)yrow32[base + j]) : 0.0;
      w[j] = (ok && !a.cold) ? wrow[base + j] : 0.0;
      mk[j] = ok ? 1.0 : 0.0;
    }
  }
  const double lb = a.lbda_vec ? a.lbda_vec[p] : a.lbda;
  const double th = lb * a.step;
  const double nstep = -a.step;

  // window rule state (wind = 6): u_{k-1} and the increments delta_{k-1}, delta_{k-2}, delta_{k-3}
  double uprev[STOP == 2 ? S : 1], d1[STOP == 2 ? S : 1], d2[STOP == 2 ? S : 1], d3[STOP == 2 ? S : 1];
  if constexpr (STOP == 2) {
#pragma unroll
    for (int j = 0; j < S; ++j) uprev[j] = d1[j] = d2[j] = d3[j] = 0.0;
  }
  bool active = live;
  int done = 0;
  double* Jrow = (WITH_J && a.J64) ? a.J64 + (int64_t)p * a.ldj : nullptr;
  float* Jrow32 = (WITH_J && !a.J64 && a.J) ? a.J + (int64_t)p * a.ldj : nullptr;

  int n_stop = a.n_iter;
  for (int it = 0;; ++it) {
    if (!WITH_J && it >= n_stop) break;
    double r[S];
    exact_forward<S, KT>(w, y, mk, taps, r);

    // ---- cost of the iterate this pass started from -------------------------
    if constexpr (WITH_J) {
      if (it > 0) {
        double sq = 0.0, l1 = 0.0;
#pragma unroll
        for (int j = 0; j < S; ++j) {
          sq = fma(r[j], r[j], sq);
          l1 += fabs(w[j]);
        }
        const double cost = seg_allsum_f64<64>(fma(0.5, sq, lb * l1));
        if (live && lane == 0 && (STOP == 0 || it <= done)) {
          if (Jrow) Jrow[it - 1] = cost;
          else if (Jrow32) Jrow32[it - 1] = (float)cost;
        }
      }
      if (it >= n_stop) break;
    }

    double num = 0.0, den = 0.0;
    exact_backward<S, KT, STOP>(r, w, taps, nstep, th, a.betas + it, uprev, d1, d2, d3, num, den);
    if constexpr (STOP != 0) {
      if (active) {
        done = it + 1;
        if (exact_stop_fires<STOP>(it, num, den, a.tol)) {
          active = false;                     // wave-uniform: one problem per wave
          n_stop = it + 1;
        }
      }
    }
  }

  if (live) {
    double* wrow = a.w + (int64_t)p * a.ldw;
#pragma unroll
    for (int j = 0; j < S; ++j)
      if (base + j < a.N) wrow[base + j] = w[j];
    if (a.n_done && lane == 0) a.n_done[p] = (STOP == 0) ? a.n_iter : done;
  }
}

// the six compiled variants of a solver (cost trace x stop rule), one switch for every form of the float64 register family:
// k(with_j, stop, grid, block, stream) launches the variant the two compile-time constants name
template <class KERNELS>
int launch_solve_variants(dim3 grid, dim3 block, bool with_j, int stop, hipStream_t st, const KERNELS& k) {
  const auto with = [&](auto sm) {
    if (with_j) k(std::true_type{}, sm, grid, block, st);
    else k(std::false_type{}, sm, grid, block, st);
  };
  if (stop == PB_STOP_NONE) with(std::integral_constant<int, 0>{});
  else if (stop == PB_STOP_LOOPS) with(std::integral_constant<int, 1>{});
  else with(std::integral_constant<int, 2>{});
  return 0;
}

template <int S, int KT>
int launch_exact(const FistaArgs& a, const double* taps, int K, bool with_j, int stop, hipStream_t st) {
  const auto td = make_taps_d<KT>(taps, K);
  const dim3 grid((unsigned)((launch_count(a) + 3) / 4)), block(256);
  return launch_solve_variants(grid, block, with_j, stop, st, [&](auto wj, auto sm, dim3 g, dim3 b, hipStream_t s) {
    hipLaunchKernelGGL((fista_exact_kernel<S, KT, decltype(wj)::value, decltype(sm)::value>), g, b, 0, s, a, td);
  });
}

}  // namespace pb
