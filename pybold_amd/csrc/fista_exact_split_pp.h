// fista_exact_split_kernel (fista_exact_split.h) and auto_lbda_split_kernel (fista_auto_split.h) with ONE HRF AND ONE
// STEP PER PROBLEM: the per-voxel-HRF call of fista_exact_pp.h for series of 641 .. 1 280 scans (S = 5 samples per lane),
// one problem over the FOUR waves of a workgroup, float64 end to end, everything in VGPRs.
//
// The pass body is the one of those kernels in its two halves (split_forward / barrier B / split_backward: shared, not
// copied), and so are the slot, problem and `live` logic, the loads, the cost trace behind barrier B, the stop rules, the
// write-out, and in the search the statistics slots stat[2][4], the AUTO_STATE slots per voxel and the init / cold / i0 /
// i1 / final_solve protocol.  What differs is where the taps and the step come from, as in fista_exact_pp.h: the
// workgroup of problem p reads its K taps from taps_pp + p * ldt (load_taps_pp: shared) and its step from step_vec[p].
// The problem index goes through readfirstlane, so both addresses are uniform and the loads are scalar loads in the
// prologue: the taps live in scalar registers, where the by-value argument of the single-HRF kernels puts them.  No more
// than K taps are read (the slots K .. ldt-1 of a row belong to the caller); the taps K .. KT-1 are 0.0 in registers.
//
// SLOT DISCIPLINE.  That of the two single-HRF kernels, unchanged: every slot of SplitLds, and of `stat` in the search,
// is written before one barrier and read behind it only, and its next write lies behind at least one further barrier.
// The taps and the step never pass through LDS.
//
// UNIFORM EXITS.  A wave that left a loop its siblings stay in would leave them waiting at a barrier for ever.  The taps,
// the step and what is derived from them (th, nstep) are read from ONE address per workgroup (p and v come from
// blockIdx.x, kernel arguments and, with a permutation, one list entry per workgroup), so they hold the same bits in the
// four waves -- and no exit reads them directly anyway.  Every return and break below depends only on
//   - the slot of the workgroup (blockIdx.x and kernel arguments) and, in the search, the state slots of the voxel (one
//     address for the four waves, written by the previous launch): the returns in the prologue, all before the first
//     barrier, taken by the workgroup as a whole;
//   - the iteration counters it / i against n_iter / n_stop / nb_sub_iter / i0 / i1 / final_solve (kernel arguments);
//   - n_stop and `done`, which change only on exact_stop_fires / auto_alpha_window_fires evaluated on sums that every wave
//     forms from the same four LDS values in the same order (split_backward behind barrier D, stat behind barrier B),
//     with tol from the kernel arguments.
// Nothing that depends on a lane, on a wave's own partial sum, on q or on the mask guards a barrier; `live` is per
// workgroup and guards stores only.
#pragma once
#include "fista_auto.h"
#include "fista_exact_pp.h"
#include "fista_exact_split.h"

namespace pb {

template <int S, int KT, bool WITH_J, int STOP>
__global__ __launch_bounds__(64 * SPLIT_WAVES) void fista_exact_split_pp_kernel(FistaArgs a) {
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
  const int p = __builtin_amdgcn_readfirstlane(slot_to_problem(a, slot, s1, live));
  const int base = (q * 64 + lane) * S;
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
  bool active = true;                               // (workgroup-uniform: a dead slot runs the same iterations, unwritten)
  int done = 0;
  double* Jrow = (WITH_J && a.J64) ? a.J64 + (int64_t)p * a.ldj : nullptr;
  float* Jrow32 = (WITH_J && !a.J64 && a.J) ? a.J + (int64_t)p * a.ldj : nullptr;

  int n_stop = a.n_iter;
  for (int it = 0;; ++it) {
    if (!WITH_J && it >= n_stop) break;
    double r[S];
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

template <int S, int KT>
int launch_exact_split_pp(const FistaArgs& a, bool with_j, int stop, hipStream_t st) {
  if (!a.taps_pp || !a.step_vec || a.K > KT || a.N > 64 * SPLIT_WAVES * S) return 1;
  const dim3 grid((unsigned)launch_count(a)), block(64 * SPLIT_WAVES);
  return launch_solve_variants(grid, block, with_j, stop, st, [&](auto wj, auto sm, dim3 g, dim3 b, hipStream_t s) {
    hipLaunchKernelGGL((fista_exact_split_pp_kernel<S, KT, decltype(wj)::value, decltype(sm)::value>), g, b, 0, s, a);
  });
}

// ---- the noise-driven lambda search with one HRF and one step per voxel, one voxel per workgroup of four waves ---------
// auto_lbda_split_kernel (fista_auto_split.h) with the same two changes; AutoArgs::step is not read.
template <int S, int KT, int STOP>
__global__ __launch_bounds__(64 * SPLIT_WAVES) void auto_lbda_split_pp_kernel(AutoArgsPP a) {
  static_assert(STOP == 0 || STOP == 2, "the search stops its inner solves on the window rule or not at all");
  static_assert(SPLIT_WAVES == 4, "the sums over the waves are written for four");
  __shared__ SplitLds<KT> lds;
  __shared__ double stat[2][SPLIT_WAVES];               // B: r^2 and |w| sums of every wave
  const int lane = threadIdx.x & 63;
  const int q = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int v = __builtin_amdgcn_readfirstlane((int)blockIdx.x);   // one voxel per workgroup
  if (v >= a.V) return;
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
  const TapsD<KT> taps = load_taps_pp<KT>(a.taps_pp, a.ld_taps, a.K, v);
  const double step = a.step_vec[v];

  const int base = (q * 64 + lane) * S;
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
    // ---- inner solve from w with the current lambda; leaves the statistics of its last iterate behind barrier B ----
    if constexpr (STOP == 2) {
#pragma unroll
      for (int j = 0; j < S; ++j) uprev[j] = d1[j] = d2[j] = d3[j] = 0.0;
    }
    const double th = lbda * step;
    int n_stop = a.nb_sub_iter, it = 0;
    for (;; ++it) {
      double r[S];
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

template <int S, int KT>
int launch_auto_split_pp(const AutoArgsPP& a, bool early_stopping, hipStream_t st) {
  if (!a.taps_pp || !a.step_vec || a.K > KT || a.N > 64 * SPLIT_WAVES * S) return 1;
  const dim3 grid((unsigned)a.V), block(64 * SPLIT_WAVES);
  if (early_stopping) hipLaunchKernelGGL((auto_lbda_split_pp_kernel<S, KT, 2>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((auto_lbda_split_pp_kernel<S, KT, 0>), grid, block, 0, st, a);
  return 0;
}

}  // namespace pb
