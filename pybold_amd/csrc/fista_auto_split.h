// The device-resident lambda search of fista_auto.h with ONE voxel over the FOUR waves of a workgroup: series of
// 641 .. 1 280 scans (S = 5 samples per lane), which the one-wave search cannot hold.  The control flow, the arguments
// (AutoArgs), the AUTO_STATE slots per voxel, the init / cold / i0 / i1 / final_solve protocol and the outputs are
// those of auto_lbda_kernel; the alpha arithmetic is its helpers (auto_alpha_update, auto_alpha_window_fires,
// auto_n_sigma2: shared, not copied, contraction off).  The inner solve is the pass of fista_exact_split_kernel in its
// two halves (fista_exact_split.h: split_forward / split_backward, shared, not copied): wave q owns the samples
// [q 64 S, (q+1) 64 S), barriers A, C and D sit inside the halves, barrier B between them belongs to this kernel.
//
//   inner loop   split_forward -> [statistics of the last pass] -> B -> leave if it >= n_stop -> split_backward.  The pass
//                that ends an inner solve runs the forward half only, so r is the residual of the last iterate, as in the
//                one-wave kernel.  The stop decision is exact_stop_fires<2> on the num / den split_backward returns: the
//                same four LDS values added in the same order in every wave.
//   statistics   on the pass with it >= n_stop only (the condition is the same in the whole workgroup): every wave sums
//                its r^2 (an fma chain over its S samples) and |w| exactly as the one-wave kernel does, reduces them with
//                seg_allsum_f64<64>, and lane 0 stores the two sums into stat[0][q], stat[1][q] BEFORE barrier B.
//                Behind B every wave forms rr = (s0 + s1) + (s2 + s3) and gg likewise, runs auto_alpha_update, shifts its
//                ring and evaluates auto_alpha_window_fires on identical bits: alpha, lbda, done, outer and n_inner are
//                the same in all four waves by construction.
//
// SLOT DISCIPLINE.  `stat` is this kernel's own (SplitLds is not grown: the LDS of fista_exact_split_kernel stays as it
// is).  Like every slot of SplitLds, stat[.][q] is written before one barrier (B) and read behind it only; its next
// write lies behind at least one further barrier -- barrier A of the next pass, which every wave crosses between
// reading stat and the statistics of the next inner solve.  The slots of SplitLds keep their own discipline
// (A -> B -> C -> D -> A ...): a pass that leaves at B skips C and D in every wave alike, and the head slots it
// published are rewritten behind the next A without having been read.
//
// UNIFORM EXITS.  A wave that left a loop its siblings stay in would leave them waiting at a barrier for ever.  Every
// return and break below depends only on blockIdx.x, kernel arguments, the state slots of the voxel (one address for the
// four waves, written by the previous launch), the iteration counters, and decisions taken on LDS-summed values that hold
// the same bits in every wave.  Nothing that depends on a lane, on a wave's own partial sum or on the mask guards a
// barrier; the workgroup of a voxel that is done returns as a whole before the first barrier.
#pragma once
#include "fista_auto.h"
#include "fista_exact_split.h"

namespace pb {

template <int S, int KT, int STOP>
__global__ __launch_bounds__(256) void auto_lbda_split_kernel(AutoArgs a, TapsD<KT> taps) {
  static_assert(STOP == 0 || STOP == 2, "the search stops its inner solves on the window rule or not at all");
  static_assert(SPLIT_WAVES == 4, "the sums over the waves are written for four");
  __shared__ SplitLds<KT> lds;
  __shared__ double stat[2][SPLIT_WAVES];               // B: r^2 and |w| sums of every wave
  const int lane = threadIdx.x & 63;
  const int q = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int v = (int)blockIdx.x;                        // one voxel per workgroup
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
  const double nstep = -a.step;
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
    const double th = lbda * a.step;
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
int launch_auto_split(const AutoArgs& a, const double* taps, int K, bool early_stopping, hipStream_t st) {
  const auto td = make_taps_d<KT>(taps, K);
  const dim3 grid((unsigned)a.V), block(64 * SPLIT_WAVES);
  if (early_stopping) hipLaunchKernelGGL((auto_lbda_split_kernel<S, KT, 2>), grid, block, 0, st, a, td);
  else hipLaunchKernelGGL((auto_lbda_split_kernel<S, KT, 0>), grid, block, 0, st, a, td);
  return 0;
}

}  // namespace pb
