// The four-wave float64 kernels (fista_exact_split.h, fista_exact_split_pp.h, fista_auto_split.h) for HRFs of up to 48 taps
// (OPT-IN: pb_fista_solve_split_long_d / _pp_d, pb_auto_lbda_split_long_d / _pp_d): series of 641 .. 1 280 scans
// (S = 5 samples per lane), one problem over the FOUR waves of a workgroup, float64 end to end, with a shared HRF or one HRF
// and one step per problem.  A 30 s HRF at the HCP TR of 0.72 s has 42 taps and an HCP run 1 200 scans: the shape the
// four-wave forms (32 taps) and the lane-held-taps forms of fista_exact_long.h (640 scans) each stop short of.
//
// The pass is the one of the four-wave kernels in its two halves (split_forward / barrier B / split_backward: shared, not
// copied -- both take the tap holder as a type parameter), and so are SplitLds, the slot, problem and `live` logic, the
// cost trace behind barrier B, the stop rules, and in the search the statistics slots stat[2][4], the AUTO_STATE slots per
// voxel, the init / cold / i0 / i1 / final_solve protocol and the alpha arithmetic (auto_alpha_update,
// auto_alpha_window_fires, auto_n_sigma2).  What differs is the home of the taps, as in fista_exact_long.h: EVERY WAVE keeps
// its own TapsLane copy (lane m of each of the four waves holds h[m], 0.0 from the K-th lane on), loaded once per launch
// with one vector load, and reads each tap with v_readlane on a constant lane where the FIR and the correlation use it.
// keep_in_lanes() stands before each half of every pass, and the mask is rebuilt per pass from one register (long_mask).
// The taps and the step never pass through LDS; nothing is read through the scalar cache.
//
// ARITHMETIC ORDER.  That of the KT = 32 four-wave kernels -- tap-major, m ascending, one fma per (tap, sample), the taps
// K .. KT-1 exactly 0.0, additions only across the waves -- so for K <= 32 every output equals theirs bit for bit: the extra
// taps add exact zeros.  The halo is wider (H = 47 samples, D = 10 lanes instead of 7): more lanes take a window value from
// the LDS tail / head of the neighbour wave instead of a DPP shift, but the value is the one its owner holds (tail + the
// owner's offset, the addition the owner performs), and the window slots beyond tap K-1 meet a tap of 0.0.
//
// SLOT DISCIPLINE.  That of the four-wave kernels, unchanged: every slot of SplitLds, and of `stat` in the search, is
// written before one barrier and read behind it only; its next write lies behind at least one further barrier
// (A -> B -> C -> D -> A ...).  SplitLds<48> is 3 136 bytes.
//
// UNIFORM EXITS.  A wave that left a loop its siblings stay in would leave them waiting at a barrier for ever.  The taps,
// the step and what is derived from them (th, nstep) are read from ONE address per workgroup (the kernel argument, or row p
// / v with p and v through readfirstlane from blockIdx.x, kernel arguments and one list entry per workgroup), so they hold
// the same bits in the four waves -- and no exit reads them.  Every return and break below depends only on
//   - the slot of the workgroup (blockIdx.x and kernel arguments) and, in the search, the state slots of the voxel (one
//     address for the four waves, written by the previous launch): the returns of the kernels' prologues and of
//     split_long_search before it loads the taps, all before the first barrier, taken by the workgroup as a whole;
//   - the iteration counters it / i against n_iter / n_stop / nb_sub_iter / i0 / i1 / final_solve (kernel arguments);
//   - n_stop and `done`, which change only on exact_stop_fires / auto_alpha_window_fires evaluated on sums that every wave
//     forms from the same four LDS values in the same order (split_backward behind barrier D, stat behind barrier B), with
//     tol from the kernel arguments.
// Nothing that depends on a lane, on a wave's own partial sum, on q, on the mask or on the tap holder guards a barrier;
// `live` is per workgroup and guards stores only.
#pragma once
#include "fista_auto.h"
#include "fista_exact_long.h"
#include "fista_exact_pp.h"
#include "fista_exact_split.h"

namespace pb {

// ---- the fixed-lambda solve of one workgroup: the body of fista_exact_split_kernel on a TapsLane ---------------------
template <int S, int KT, bool WITH_J, int STOP>
__device__ __forceinline__ void split_long_solve(const FistaArgs& a, int p, bool live, double step, TapsLane taps,
                                                 SplitLds<KT>& lds, int q, int lane) {
  const int base = (q * 64 + lane) * S;
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
  bool active = true;                               // (workgroup-uniform: a dead slot runs the same iterations, unwritten)
  int done = 0;
  double* Jrow = (WITH_J && a.J64) ? a.J64 + (int64_t)p * a.ldj : nullptr;
  float* Jrow32 = (WITH_J && !a.J64 && a.J) ? a.J + (int64_t)p * a.ldj : nullptr;

  int n_stop = a.n_iter;
  for (int it = 0;; ++it) {
    if (!WITH_J && it >= n_stop) break;
    double r[S], mk[S];
    long_mask<S>(n_own, mk);
    taps.keep_in_lanes();
    split_forward<S, KT>(w, y, mk, taps, r, lds, q, lane);

    // ---- cost of the iterate this pass started from: partial sums behind barrier B ----
    if constexpr (WITH_J) {
      if (it > 0) {
        double sq = 0.0, l1 = 0.0;
#pragma unroll
        for (int j = 0; j < S; ++j) {
          sq = fma(r[j], r[j], sq);
          l1 += fabs(w[j]);
        }
        const double part = seg_allsum_f64<64>(fma(0.5, sq, lb * l1));
        if (lane == 0) lds.part[q] = part;
      }
    }
    __syncthreads();                                                    // ---- B
    if constexpr (WITH_J) {
      if (it > 0) {
        const double cost = (lds.part[0] + lds.part[1]) + (lds.part[2] + lds.part[3]);
        if (live && threadIdx.x == 0 && (STOP == 0 || it <= done)) {
          if (Jrow) Jrow[it - 1] = cost;
          else if (Jrow32) Jrow32[it - 1] = (float)cost;
        }
      }
      if (it >= n_stop) break;
    }

    double num = 0.0, den = 0.0;
    taps.keep_in_lanes();
    split_backward<S, KT, STOP>(r, w, taps, nstep, th, a.betas + it, uprev, d1, d2, d3, num, den, lds, q, lane);
    if constexpr (STOP != 0) {
      if (active) {
        done = it + 1;
        // (the same four LDS values added in the same order in every wave: one decision for the workgroup)
        if (__builtin_amdgcn_readfirstlane((int)exact_stop_fires<STOP>(it, num, den, a.tol))) {
          active = false;
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
    if (a.n_done && threadIdx.x == 0) a.n_done[p] = (STOP == 0) ? a.n_iter : done;
  }
}

template <int S, int KT, bool WITH_J, int STOP>
__global__ __launch_bounds__(64 * SPLIT_WAVES) void fista_exact_split_long_kernel(FistaArgs a, TapsD<KT> td) {
  static_assert(SPLIT_WAVES == 4, "the sums over the waves are written for four");
  __shared__ SplitLds<KT> lds;
  const int lane = threadIdx.x & 63;
  const int q = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // one slot of this launch's list per WORKGROUP: everything up to `live` is the same in its four waves, so the
  // workgroup of an empty candidate launch leaves as a whole
  int s0, s1;
  launch_slots(a, s0, s1);
  const int slot = (int)blockIdx.x + s0;
  if (slot >= s1 && a.range) return;
  bool live;
  const int p = slot_to_problem(a, slot, s1, live);
  split_long_solve<S, KT, WITH_J, STOP>(a, p, live, a.step, taps_lane_from_arg<KT>(td, lane), lds, q, lane);
}

template <int S, int KT, bool WITH_J, int STOP>
__global__ __launch_bounds__(64 * SPLIT_WAVES) void fista_exact_split_long_pp_kernel(FistaArgs a) {
  static_assert(SPLIT_WAVES == 4, "the sums over the waves are written for four");
  __shared__ SplitLds<KT> lds;
  const int lane = threadIdx.x & 63;
  const int q = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  int s0, s1;
  launch_slots(a, s0, s1);
  const int slot = (int)blockIdx.x + s0;
  if (slot >= s1 && a.range) return;
  bool live;
  const int p = __builtin_amdgcn_readfirstlane(slot_to_problem(a, slot, s1, live));
  // (the first K slots of row p in one vector load per wave: the slots K .. ldt-1 belong to the caller and are not read)
  split_long_solve<S, KT, WITH_J, STOP>(a, p, live, a.step_vec[p], taps_lane_from_row(a.taps_pp, a.ldt, a.K, p, lane), lds, q,
                                        lane);
}

template <int S, int KT>
int launch_exact_split_long(const FistaArgs& a, const double* taps, int K, bool with_j, int stop, hipStream_t st) {
  if (!taps || K > KT || a.N > 64 * SPLIT_WAVES * S) return 1;
  const auto td = make_taps_d<KT>(taps, K);
  const dim3 grid((unsigned)launch_count(a));
  return launch_solve_variants(grid, dim3(64 * SPLIT_WAVES), with_j, stop, st, [&](auto wj, auto sm, dim3 g, dim3 b, hipStream_t s) {
    hipLaunchKernelGGL((fista_exact_split_long_kernel<S, KT, decltype(wj)::value, decltype(sm)::value>), g, b, 0, s, a, td);
  });
}

template <int S, int KT>
int launch_exact_split_long_pp(const FistaArgs& a, bool with_j, int stop, hipStream_t st) {
  if (!a.taps_pp || !a.step_vec || a.K > KT || a.N > 64 * SPLIT_WAVES * S) return 1;
  const dim3 grid((unsigned)launch_count(a));
  return launch_solve_variants(grid, dim3(64 * SPLIT_WAVES), with_j, stop, st, [&](auto wj, auto sm, dim3 g, dim3 b, hipStream_t s) {
    hipLaunchKernelGGL((fista_exact_split_long_pp_kernel<S, KT, decltype(wj)::value, decltype(sm)::value>), g, b, 0, s, a);
  });
}

// ---- the lambda search of one workgroup: the body of auto_lbda_split_kernel on a TapsLane ----------------------------
// `load` returns the voxel's (step, taps) and is called after the voxel's done flag has been read (as in long_search_wave):
// the workgroup of a voxel that has left the search loads nothing more
template <int S, int KT, int STOP, class LOAD>
__device__ __forceinline__ void split_long_search(const AutoArgs& a, int v, const LOAD& load, SplitLds<KT>& lds,
                                                  double (&stat)[2][SPLIT_WAVES], int q, int lane) {
  static_assert(STOP == 0 || STOP == 2, "the search stops its inner solves on the window rule or not at all");
  double* st = a.work + (int64_t)v * AUTO_STATE;
  long long* sti = reinterpret_cast<long long*>(st);

  double alpha = 1.0, lbda = 0.5, ring[AUTO_WIND];
  long long n_inner = 0;
  int outer = 0, done = 0;
#pragma unroll
  for (int k = 0; k < AUTO_WIND; ++k) ring[k] = 0.0;
  if (!a.init) {
    done = __builtin_amdgcn_readfirstlane((int)sti[9]);
    if (done && !a.final_solve) return;                 // this voxel left the search in an earlier launch: all four waves
    alpha = st[0];
    lbda = st[1];
#pragma unroll
    for (int k = 0; k < AUTO_WIND; ++k) ring[k] = st[2 + k];
    outer = __builtin_amdgcn_readfirstlane((int)sti[8]);
    n_inner = sti[10];
  }
  double step;
  TapsLane taps = load(step);

  const int base = (q * 64 + lane) * S;
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
    // ---- inner solve from w with the current lambda; leaves the statistics of its last iterate behind barrier B ----
    if constexpr (STOP == 2) {
#pragma unroll
      for (int j = 0; j < S; ++j) uprev[j] = d1[j] = d2[j] = d3[j] = 0.0;
    }
    const double th = lbda * step;
    int n_stop = a.nb_sub_iter, it = 0;
    for (;; ++it) {
      double r[S], mk[S];
      long_mask<S>(n_own, mk);
      taps.keep_in_lanes();
      split_forward<S, KT>(w, y, mk, taps, r, lds, q, lane);
      if (it >= n_stop && !last) {                      // (the same in the whole workgroup)
        double sq = 0.0, l1 = 0.0;
#pragma unroll
        for (int j = 0; j < S; ++j) {
          sq = fma(r[j], r[j], sq);
          l1 += fabs(w[j]);
        }
        sq = seg_allsum_f64<64>(sq);
        l1 = seg_allsum_f64<64>(l1);
        if (lane == 0) {
          stat[0][q] = sq;
          stat[1][q] = l1;
        }
      }
      __syncthreads();                                                    // ---- B
      if (it >= n_stop) break;
      double num = 0.0, den = 0.0;
      taps.keep_in_lanes();
      split_backward<S, KT, STOP>(r, w, taps, nstep, th, a.betas + it, uprev, d1, d2, d3, num, den, lds, q, lane);
      if constexpr (STOP == 2) {
        // (the same four LDS values added in the same order in every wave: one decision for the workgroup)
        if (__builtin_amdgcn_readfirstlane((int)exact_stop_fires<2>(it, num, den, a.tol))) n_stop = it + 1;
      }
    }
    n_inner += it;
    if (last) break;
    // ---- residual statistics over the four waves, alpha update, alpha window: identical bits in every wave ----
    const double rr = (stat[0][0] + stat[0][1]) + (stat[0][2] + stat[0][3]);
    const double gg = (stat[1][0] + stat[1][1]) + (stat[1][2] + stat[1][3]);
    double cost;
    auto_alpha_update(rr, gg, n_sigma2, alpha, lbda, cost);
#pragma unroll
    for (int k = 0; k + 1 < AUTO_WIND; ++k) ring[k] = ring[k + 1];
    ring[AUTO_WIND - 1] = alpha;
    if (threadIdx.x == 0) {
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
  if (threadIdx.x == 0) {
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
__global__ __launch_bounds__(64 * SPLIT_WAVES) void auto_lbda_split_long_kernel(AutoArgs a, TapsD<KT> td) {
  static_assert(SPLIT_WAVES == 4, "the sums over the waves are written for four");
  __shared__ SplitLds<KT> lds;
  __shared__ double stat[2][SPLIT_WAVES];               // B: r^2 and |w| sums of every wave
  const int lane = threadIdx.x & 63;
  const int q = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int v = (int)blockIdx.x;                        // one voxel per workgroup
  if (v >= a.V) return;
  split_long_search<S, KT, STOP>(a, v, [&](double& step) {
    step = a.step;
    return taps_lane_from_arg<KT>(td, lane);
  }, lds, stat, q, lane);
}

template <int S, int KT, int STOP>
__global__ __launch_bounds__(64 * SPLIT_WAVES) void auto_lbda_split_long_pp_kernel(AutoArgsPP a) {
  static_assert(SPLIT_WAVES == 4, "the sums over the waves are written for four");
  __shared__ SplitLds<KT> lds;
  __shared__ double stat[2][SPLIT_WAVES];               // B: r^2 and |w| sums of every wave
  const int lane = threadIdx.x & 63;
  const int q = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int v = __builtin_amdgcn_readfirstlane((int)blockIdx.x);   // one voxel per workgroup
  if (v >= a.V) return;
  split_long_search<S, KT, STOP>(a, v, [&](double& step) {
    step = a.step_vec[v];
    return taps_lane_from_row(a.taps_pp, a.ld_taps, a.K, v, lane);
  }, lds, stat, q, lane);
}

template <int S, int KT>
int launch_auto_split_long(const AutoArgs& a, const double* taps, int K, bool early_stopping, hipStream_t st) {
  if (!taps || K > KT || a.N > 64 * SPLIT_WAVES * S) return 1;
  const auto td = make_taps_d<KT>(taps, K);
  const dim3 grid((unsigned)a.V), block(64 * SPLIT_WAVES);
  if (early_stopping) hipLaunchKernelGGL((auto_lbda_split_long_kernel<S, KT, 2>), grid, block, 0, st, a, td);
  else hipLaunchKernelGGL((auto_lbda_split_long_kernel<S, KT, 0>), grid, block, 0, st, a, td);
  return 0;
}

template <int S, int KT>
int launch_auto_split_long_pp(const AutoArgsPP& a, bool early_stopping, hipStream_t st) {
  if (!a.taps_pp || !a.step_vec || a.K > KT || a.N > 64 * SPLIT_WAVES * S) return 1;
  const dim3 grid((unsigned)a.V), block(64 * SPLIT_WAVES);
  if (early_stopping) hipLaunchKernelGGL((auto_lbda_split_long_pp_kernel<S, KT, 2>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((auto_lbda_split_long_pp_kernel<S, KT, 0>), grid, block, 0, st, a);
  return 0;
}

}  // namespace pb
