// fista_exact_kernel (fista_exact.h) and auto_lbda_kernel (fista_auto.h) with ONE HRF AND ONE STEP PER PROBLEM: the
// last step of the reference's per-voxel workflow -- bd on every voxel, then deconv of every voxel with its own
// estimated HRF (examples/icassp_2019/simulation.py:62-72) -- in float64 end to end, one problem per wave64, four
// waves per workgroup, everything in VGPRs.
//
// The pass body is the one of those kernels (exact_forward / exact_backward, shared, not copied).  What differs is where
// the taps come from: wave p reads its K taps from a.taps_pp + p * a.ldt and its step from a.step_vec[p].  The problem
// index goes through readfirstlane, so both addresses are uniform over the wave and the loads are scalar loads: the
// taps live in scalar registers, where the by-value kernel argument of fista_exact_kernel puts them, not in 2 * KT
// more VGPRs.  No more than K taps are read (the slots K .. ldt-1 of a row belong to the caller and may hold anything);
// the taps K .. KT-1 are 0.0 in registers.
#pragma once
#include "fista_auto.h"
#include "fista_exact.h"

namespace pb {

// the taps of problem p (uniform over the wave): index clamped to tap 0 beyond K, value replaced by 0.0 -- no branch,
// no read past the K-th tap
template <int KT>
__device__ __forceinline__ TapsD<KT> load_taps_pp(const double* taps_pp, int64_t ldt, int K, int p) {
  const double* tp = taps_pp + (int64_t)p * ldt;
  TapsD<KT> t;
  static_for<0, KT>([&](auto mc) {
    constexpr int m = decltype(mc)::value;
    const double h = tp[m < K ? m : 0];
    t.h[m] = m < K ? h : 0.0;
  });
  return t;
}

template <int S, int KT, bool WITH_J, int STOP>
__global__ __launch_bounds__(256) void fista_exact_pp_kernel(FistaArgs a) {
  const int lane = threadIdx.x & 63;
  int s0, s1;
  launch_slots(a, s0, s1);
  const int slot = (int)((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) + s0;
  if (slot >= s1 && a.range) return;               // (one problem per wave: uniform)
  bool live;
  const int p = __builtin_amdgcn_readfirstlane(slot_to_problem(a, slot, s1, live));
  const int base = lane * S;
  const TapsD<KT> taps = load_taps_pp<KT>(a.taps_pp, a.ldt, a.K, p);
  const double step = a.step_vec[p];

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

template <int S, int KT>
int launch_exact_pp(const FistaArgs& a, bool with_j, int stop, hipStream_t st) {
  if (!a.taps_pp || !a.step_vec || a.K > KT) return 1;
  const dim3 grid((unsigned)((launch_count(a) + 3) / 4)), block(256);
  return launch_solve_variants(grid, block, with_j, stop, st, [&](auto wj, auto sm, dim3 g, dim3 b, hipStream_t s) {
    hipLaunchKernelGGL((fista_exact_pp_kernel<S, KT, decltype(wj)::value, decltype(sm)::value>), g, b, 0, s, a);
  });
}

// ---- the noise-driven lambda search with one HRF and one step per voxel ---------------------------------------------
// auto_lbda_kernel (fista_auto.h) with the same two changes; the state slots, the launch protocol, auto_alpha_update and
// auto_alpha_window_fires are its own.  AutoArgs::step is not read.
struct AutoArgsPP : AutoArgs {
  const double* taps_pp;            // [V][ld_taps], K used
  int64_t ld_taps;
  const double* step_vec;           // [V]
  int K;
};

template <int S, int KT, int STOP>
__global__ __launch_bounds__(256) void auto_lbda_pp_kernel(AutoArgsPP a) {
  static_assert(STOP == 0 || STOP == 2, "the search stops its inner solves on the window rule or not at all");
  const int lane = threadIdx.x & 63;
  const int v = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
  if (v >= a.V) return;                                 // (one voxel per wave: uniform)
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
  const TapsD<KT> taps = load_taps_pp<KT>(a.taps_pp, a.ld_taps, a.K, v);
  const double step = a.step_vec[v];

  const int base = lane * S;
  double y[S], w[S], mk[S];
  {
    const double* yrow = a.y + (int64_t)v * a.ldy;
    const double* wrow = a.w + (int64_t)v * a.ldw;
    const bool zero = a.init && a.cold;
#pragma unroll
    for (int j = 0; j < S; ++j) {
      const bool ok = base + j < a.N;
      y[j] = ok ? yrow[base + j] : 0.0;
      w[j] = (ok && !zero) ? wrow[base + j] : 0.0;
      mk[j] = ok ? 1.0 : 0.0;
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
      exact_forward<S, KT>(w, y, mk, taps, r);
      if (it >= n_stop) break;
      double num = 0.0, den = 0.0;
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

template <int S, int KT>
int launch_auto_pp(const AutoArgsPP& a, bool early_stopping, hipStream_t st) {
  if (!a.taps_pp || !a.step_vec || a.K > KT) return 1;
  const dim3 grid((unsigned)((a.V + 3) / 4)), block(256);
  if (early_stopping) hipLaunchKernelGGL((auto_lbda_pp_kernel<S, KT, 2>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((auto_lbda_pp_kernel<S, KT, 0>), grid, block, 0, st, a);
  return 0;
}

}  // namespace pb
