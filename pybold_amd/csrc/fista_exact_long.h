// fista_exact_kernel (fista_exact.h) and auto_lbda_kernel (fista_auto.h) for HRFs of up to 48 taps (OPT-IN: PB_FLAG_LONG_HRF,
// pb_auto_lbda_long_d, pb_auto_lbda_long_pp_d): float64 end to end, one problem per wave64, S = 5 / 10 samples per lane
// (series of up to 320 / 640 scans), with a shared HRF or one HRF and one step per problem.
//
// The pass is the one of those kernels (exact_forward / exact_backward / exact_stop_fires, shared, not copied), and the
// search keeps their state slots, launch protocol and alpha arithmetic (auto_alpha_update, auto_alpha_window_fires,
// auto_n_sigma2).  What differs is the home of the taps.  There they are a by-value kernel argument (or scalar loads) and
// live in scalar registers: 32 float64 taps fill the scalar file, 48 spill 61 .. 143 SGPRs into VGPR lanes.  Here ONE
// VGPR PAIR of the wave holds them (TapsLane: lane m keeps h[m], 0.0 from the K-th lane on; 48 <= 64), loaded once per
// launch, and each tap is read where the FIR and the correlation use it, with v_readlane_b32 on a constant lane: a
// scalar pair that lives for the S fused multiply-adds of that tap and no longer.  The scalar file never carries the taps.
//
// Arithmetic order is that of the KT = 32 kernels -- tap-major, m ascending, one fma per (tap, sample), the taps
// K .. KT-1 exactly 0.0 -- so for K <= 32 every output equals theirs bit for bit: the extra taps add exact zeros.
#pragma once
#include "fista_auto.h"
#include "fista_exact.h"
#include "fista_exact_pp.h"

namespace pb {

struct TapsLane {
  double v;                                   // lane m: h[m]
  template <int m>
  __device__ __forceinline__ double tap() const {
    static_assert(m >= 0 && m < 64, "one tap per lane of the wave");
    return readlane_f64(v, m);
  }
  // Before each half of a pass: the holder becomes a value the compiler knows nothing about, so the reads above stay
  // where they are used.  Without it they are loop-invariant, all 2 * KT of them are hoisted in front of the iteration
  // loop, and the taps are back in the scalar file (and from there in spill lanes).  No instruction is emitted.
  __device__ __forceinline__ void keep_in_lanes() { asm volatile("" : "+v"(v)); }
};

// shared HRF: from the by-value kernel argument (taps K .. KT-1 are 0.0 there: make_taps_d)
template <int KT>
__device__ __forceinline__ TapsLane taps_lane_from_arg(const TapsD<KT>& td, int lane) {
  static_assert(KT <= 64, "one tap per lane of the wave");
  TapsLane t;
  t.v = lane < KT ? td.h[lane < KT ? lane : 0] : 0.0;     // one vector load from the argument segment
  return t;
}

// one HRF per problem: ONE vector load of the row's first K slots (the slots K .. ldt-1 belong to the caller and are not read)
__device__ __forceinline__ TapsLane taps_lane_from_row(const double* taps_pp, int64_t ldt, int K, int p, int lane) {
  TapsLane t;
  t.v = lane < K ? taps_pp[(int64_t)p * ldt + lane] : 0.0;
  return t;
}

// The mask of the lane's samples inside the series (1.0 / 0.0, what exact_forward multiplies the residual by), rebuilt for
// every pass from ONE register: kept as S loop-invariant float64 it costs 2 S VGPRs, and beside the window of a 48-tap
// pass the S = 10 search had none left (four of them went to spill slots).  The same values, so the same bits.
template <int S>
__device__ __forceinline__ void long_mask(int n_own, double (&mk)[S]) {
  asm volatile("" : "+v"(n_own));             // (not loop-invariant to the compiler: see TapsLane::keep_in_lanes)
#pragma unroll
  for (int j = 0; j < S; ++j) mk[j] = j < n_own ? 1.0 : 0.0;
}

// ---- the fixed-lambda solve of one wave: the body of fista_exact_kernel on a TapsLane ----------------------------------
template <int S, int KT, bool WITH_J, int STOP>
__device__ __forceinline__ void long_solve_wave(const FistaArgs& a, int p, bool live, double step, TapsLane taps) {
  const int lane = threadIdx.x & 63;
  const int base = lane * S;
  const int n_own = a.N - base;                // samples of the series from the lane's first on (<= 0: none)
  double y[S], w[S];
  {
    const double* yrow = a.y64 ? a.y64 + (int64_t)(p / a.y_rep) * a.ldy : nullptr;
    const float* yrow32 = a.y64 ? nullptr : a.y + (int64_t)(p / a.y_rep) * a.ldy;
    const double* wrow = a.w + (int64_t)p * a.ldw;
#pragma unroll
    for (int j = 0; j < S; ++j) {
      const bool ok = base + j < a.N;
      y[j] = ok ? (yrow ? yrow[base + j] : (double)yrow32[base + j]) : 0.0;
      w[j] = (ok && !a.cold) ? wrow[base + j] : 0.0;
    }
  }
  const double lb = a.lbda_vec ? a.lbda_vec[p] : a.lbda;
  const double th = lb * step;
  const double nstep = -step;

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
    double r[S], mk[S];
    long_mask<S>(n_own, mk);
    taps.keep_in_lanes();
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
    taps.keep_in_lanes();
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

template <int S, int KT, bool WITH_J, int STOP>
__global__ __launch_bounds__(256) void fista_exact_long_kernel(FistaArgs a, TapsD<KT> td) {
  int s0, s1;
  launch_slots(a, s0, s1);
  const int slot = (int)((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) + s0;
  if (slot >= s1 && a.range) return;               // (one problem per wave: uniform)
  bool live;
  const int p = slot_to_problem(a, slot, s1, live);
  long_solve_wave<S, KT, WITH_J, STOP>(a, p, live, a.step, taps_lane_from_arg<KT>(td, threadIdx.x & 63));
}

template <int S, int KT, bool WITH_J, int STOP>
__global__ __launch_bounds__(256) void fista_exact_long_pp_kernel(FistaArgs a) {
  int s0, s1;
  launch_slots(a, s0, s1);
  const int slot = (int)((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) + s0;
  if (slot >= s1 && a.range) return;               // (one problem per wave: uniform)
  bool live;
  const int p = __builtin_amdgcn_readfirstlane(slot_to_problem(a, slot, s1, live));
  long_solve_wave<S, KT, WITH_J, STOP>(a, p, live, a.step_vec[p], taps_lane_from_row(a.taps_pp, a.ldt, a.K, p, threadIdx.x & 63));
}

template <int S, int KT>
int launch_exact_long(const FistaArgs& a, const double* taps, int K, bool with_j, int stop, hipStream_t st) {
  if (!taps || K > KT) return 1;
  const auto td = make_taps_d<KT>(taps, K);
  const dim3 grid((unsigned)((launch_count(a) + 3) / 4));
  return launch_solve_variants(grid, dim3(256), with_j, stop, st, [&](auto wj, auto sm, dim3 g, dim3 b, hipStream_t s) {
    hipLaunchKernelGGL((fista_exact_long_kernel<S, KT, decltype(wj)::value, decltype(sm)::value>), g, b, 0, s, a, td);
  });
}

template <int S, int KT>
int launch_exact_long_pp(const FistaArgs& a, bool with_j, int stop, hipStream_t st) {
  if (!a.taps_pp || !a.step_vec || a.K > KT) return 1;
  const dim3 grid((unsigned)((launch_count(a) + 3) / 4));
  return launch_solve_variants(grid, dim3(256), with_j, stop, st, [&](auto wj, auto sm, dim3 g, dim3 b, hipStream_t s) {
    hipLaunchKernelGGL((fista_exact_long_pp_kernel<S, KT, decltype(wj)::value, decltype(sm)::value>), g, b, 0, s, a);
  });
}

// ---- the lambda search of one wave: the body of auto_lbda_kernel on a TapsLane ----------------------------------------
// `load` returns the voxel's (step, taps) and is called after the voxel's done flag has been read: a wave whose voxel has
// left the search loads nothing more
template <int S, int KT, int STOP, class LOAD>
__device__ __forceinline__ void long_search_wave(const AutoArgs& a, int v, const LOAD& load) {
  static_assert(STOP == 0 || STOP == 2, "the search stops its inner solves on the window rule or not at all");
  const int lane = threadIdx.x & 63;
  double* st = a.work + (int64_t)v * AUTO_STATE;
  long long* sti = reinterpret_cast<long long*>(st);

  double alpha = 1.0, lbda = 0.5, ring[AUTO_WIND];
  long long n_inner = 0;
  int outer = 0, done = 0;
#pragma unroll
  for (int k = 0; k < AUTO_WIND; ++k) ring[k] = 0.0;
  if (!a.init) {
    done = __builtin_amdgcn_readfirstlane((int)sti[9]);
    if (done && !a.final_solve) return;                 // this voxel left the search in an earlier launch
    alpha = st[0];
    lbda = st[1];
#pragma unroll
    for (int k = 0; k < AUTO_WIND; ++k) ring[k] = st[2 + k];
    outer = __builtin_amdgcn_readfirstlane((int)sti[8]);
    n_inner = sti[10];
  }
  double step;
  TapsLane taps = load(step);

  const int base = lane * S;
  const int n_own = a.N - base;                // samples of the series from the lane's first on (<= 0: none)
  double y[S], w[S];
  {
    const double* yrow = a.y + (int64_t)v * a.ldy;
    const double* wrow = a.w + (int64_t)v * a.ldw;
    const bool zero = a.init && a.cold;
#pragma unroll
    for (int j = 0; j < S; ++j) {
      const bool ok = base + j < a.N;
      y[j] = ok ? yrow[base + j] : 0.0;
      w[j] = (ok && !zero) ? wrow[base + j] : 0.0;
    }
  }
  const double nstep = -step;
  const double n_sigma2 = auto_n_sigma2(a.N, a.sigma[v]);
  double* Rrow = a.R ? a.R + (int64_t)v * a.ldt : nullptr;
  double* Grow = a.G ? a.G + (int64_t)v * a.ldt : nullptr;
  double* Jrow = a.J ? a.J + (int64_t)v * a.ldt : nullptr;

  double uprev[STOP == 2 ? S : 1], d1[STOP == 2 ? S : 1], d2[STOP == 2 ? S : 1], d3[STOP == 2 ? S : 1];
  int i = a.i0;
  for (;;) {
    const bool last = done || i >= a.i1;                // no outer iteration left in this launch: the final solve, or out
    if (last && !a.final_solve) break;
    // ---- inner solve from w with the current lambda; leaves r = the residual of its last iterate ----
    if constexpr (STOP == 2) {
#pragma unroll
      for (int j = 0; j < S; ++j) uprev[j] = d1[j] = d2[j] = d3[j] = 0.0;
    }
    const double th = lbda * step;
    double r[S];
    int n_stop = a.nb_sub_iter, it = 0;
    for (;; ++it) {
      double mk[S];
      long_mask<S>(n_own, mk);
      taps.keep_in_lanes();
      exact_forward<S, KT>(w, y, mk, taps, r);
      if (it >= n_stop) break;
      double num = 0.0, den = 0.0;
      taps.keep_in_lanes();
      exact_backward<S, KT, STOP>(r, w, taps, nstep, th, a.betas + it, uprev, d1, d2, d3, num, den);
      if constexpr (STOP == 2) {
        if (__builtin_amdgcn_readfirstlane((int)exact_stop_fires<2>(it, num, den, a.tol))) n_stop = it + 1;
      }
    }
    n_inner += it;
    if (last) break;
    // ---- residual statistics, alpha update, alpha window ----
    double sq = 0.0, l1 = 0.0;
#pragma unroll
    for (int j = 0; j < S; ++j) {
      sq = fma(r[j], r[j], sq);
      l1 += fabs(w[j]);
    }
    const double rr = seg_allsum_f64<64>(sq), gg = seg_allsum_f64<64>(l1);
    double cost;
    auto_alpha_update(rr, gg, n_sigma2, alpha, lbda, cost);
#pragma unroll
    for (int k = 0; k + 1 < AUTO_WIND; ++k) ring[k] = ring[k + 1];
    ring[AUTO_WIND - 1] = alpha;
    if (lane == 0) {
      if (Rrow) Rrow[i] = rr;
      if (Grow) Grow[i] = gg;
      if (Jrow) Jrow[i] = cost;
    }
    if constexpr (STOP == 2) {
      if (i > AUTO_WIND) done = __builtin_amdgcn_readfirstlane((int)auto_alpha_window_fires(ring, a.tol));
    }
    ++i;
    outer = i;
  }

  double* wrow = a.w + (int64_t)v * a.ldw;
#pragma unroll
  for (int j = 0; j < S; ++j)
    if (base + j < a.N) wrow[base + j] = w[j];
  if (lane == 0) {
    st[0] = alpha;
    st[1] = lbda;
#pragma unroll
    for (int k = 0; k < AUTO_WIND; ++k) st[2 + k] = ring[k];
    sti[8] = outer;
    sti[9] = done;
    sti[10] = n_inner;
    if (a.final_solve) {
      if (a.alpha_out) a.alpha_out[v] = alpha;
      if (a.lbda_out) a.lbda_out[v] = lbda;
      if (a.n_outer) a.n_outer[v] = outer;
      if (a.n_inner) a.n_inner[v] = n_inner;
    }
  }
}

template <int S, int KT, int STOP>
__global__ __launch_bounds__(256) void auto_lbda_long_kernel(AutoArgs a, TapsD<KT> td) {
  const int v = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (v >= a.V) return;                                 // (one voxel per wave: uniform)
  long_search_wave<S, KT, STOP>(a, v, [&](double& step) {
    step = a.step;
    return taps_lane_from_arg<KT>(td, threadIdx.x & 63);
  });
}

template <int S, int KT, int STOP>
__global__ __launch_bounds__(256) void auto_lbda_long_pp_kernel(AutoArgsPP a) {
  const int v = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
  if (v >= a.V) return;                                 // (one voxel per wave: uniform)
  long_search_wave<S, KT, STOP>(a, v, [&](double& step) {
    step = a.step_vec[v];
    return taps_lane_from_row(a.taps_pp, a.ld_taps, a.K, v, threadIdx.x & 63);
  });
}

template <int S, int KT>
int launch_auto_long(const AutoArgs& a, const double* taps, int K, bool early_stopping, hipStream_t st) {
  if (!taps || K > KT) return 1;
  const auto td = make_taps_d<KT>(taps, K);
  const dim3 grid((unsigned)((a.V + 3) / 4)), block(256);
  if (early_stopping) hipLaunchKernelGGL((auto_lbda_long_kernel<S, KT, 2>), grid, block, 0, st, a, td);
  else hipLaunchKernelGGL((auto_lbda_long_kernel<S, KT, 0>), grid, block, 0, st, a, td);
  return 0;
}

template <int S, int KT>
int launch_auto_long_pp(const AutoArgsPP& a, bool early_stopping, hipStream_t st) {
  if (!a.taps_pp || !a.step_vec || a.K > KT) return 1;
  const dim3 grid((unsigned)((a.V + 3) / 4)), block(256);
  if (early_stopping) hipLaunchKernelGGL((auto_lbda_long_pp_kernel<S, KT, 2>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((auto_lbda_long_pp_kernel<S, KT, 0>), grid, block, 0, st, a);
  return 0;
}

}  // namespace pb
