// The all-float64 register-resident FISTA kernel (fista_exact.h) with ONE series over the FOUR waves of a workgroup:
// series of 641 .. 1 280 scans (S = 5 samples per lane), the run length of an HCP session, which the one-wave form
// (S <= 10: 640 scans) cannot hold and which ran on the any-size LDS kernel (generic.h) instead.
//
// Wave q owns the samples [q 64 S, (q+1) 64 S) and runs the one-wave pass on them with the per-lane code of
// fista_exact.h (exact_window_below / _above, exact_fir_residual, exact_corr_suffix, exact_update: shared, not copied).
// What crosses a wave boundary goes through SplitLds (~2 KB) and workgroup barriers, four per iteration at most:
//
//   A  prefix         every wave publishes the last H = KT-1 values of its LOCAL cumsum (the last of them is its total).
//                     Behind the barrier wave q adds the totals of the waves below it in ascending order, ONE addition
//                     per sample, and the lanes whose DPP shift ran off the wave take their halo from the tail of wave
//                     q-1 plus the offset of wave q-1: the addition the owner performs, so halo and owner agree bit for bit.
//   B  residual halo  the first H residuals of wave q+1 go to wave q (the correlation reads ahead); the partial sums of
//                     the cost trace travel behind the same barrier.  B sits BETWEEN the two halves and belongs to the
//                     caller: split_forward publishes, the caller synchronises, split_backward reads.
//   C  suffix         every wave publishes the total of g; wave q adds the totals of the waves above it, from the top
//                     down, by additions only: above the last sample of the series the sum is EXACTLY 0, as in
//                     wave_suffix_excl_f64 (fista_exact.h) -- the reference's prox for a negative threshold is
//                     discontinuous there, and so is a series such as N = 641 whose upper waves hold padding only.
//   D  stop sums      (STOP != 0) every wave publishes its two partial sums; every wave adds the four partials in the same
//                     order, so all four hold the same bits and take the same decision.
//
// Every slot of SplitLds is written before one barrier and read behind it only; its next write lies behind at least one
// further barrier (A -> B -> C -> D -> A ...), so no slot needs a second copy.
//
// UNIFORM EXITS.  A wave that left a loop its siblings stay in would leave them waiting at a barrier for ever.  Every exit
// depends on values that are the same in the whole workgroup by construction: the slot of the workgroup (blockIdx.x and
// kernel arguments), the iteration counter and n_iter, and the stop decision, which every wave evaluates on the same four
// LDS values in the same order.  Nothing that differs between waves or lanes (the mask, `live` is per workgroup) guards a
// barrier.
#pragma once
#include "fista_exact.h"

namespace pb {

constexpr int SPLIT_WAVES = 4;

template <int KT>
struct SplitLds {
  double tail[SPLIT_WAVES][KT - 1];       // A: last H local cumsum values of every wave
  double head[SPLIT_WAVES][KT - 1];       // B: first H residuals of every wave
  double part[SPLIT_WAVES];               // B: partial sums of the cost
  double gtot[SPLIT_WAVES];               // C: wave totals of g
  double num[SPLIT_WAVES], den[SPLIT_WAVES];   // D: partial sums of the stop criterion
};

// Both halves read the taps through a HOLDER (fista_exact.h: TapsD, the by-value argument in scalar registers; TapsLane of
// fista_exact_long.h, one VGPR pair of every wave, for the 48-tap kernels of fista_exact_split_long.h).
//
// forward half: z = cumsum(w) over the whole series, r = (h * z - y) on the samples of this wave; leaves the head of r in
// LDS for the wave below.  Holds barrier A; the caller places barrier B behind it.
template <int S, int KT, class TAPS>
__device__ __forceinline__ void split_forward(const double (&w)[S], const double (&y)[S], const double (&mk)[S],
                                              const TAPS& taps, double (&r)[S], SplitLds<KT>& lds, int q, int lane) {
  constexpr int H = KT - 1;
  constexpr int D = (H + S - 1) / S;
  static_assert(H >= 1 && H <= 64 * S, "the halo comes from the neighbour wave alone");
  // ---- z = cumsum(w) within the wave -------------------------------------
  double z[S];
  z[0] = w[0];
#pragma unroll
  for (int j = 1; j < S; ++j) z[j] = z[j - 1] + w[j];
  {
    const double off = dpp_f64<DPP_WAVE_SHR1>(wave_prefix_incl_f64(z[S - 1]));
#pragma unroll
    for (int j = 0; j < S; ++j) z[j] += off;
  }
  if (lane >= 64 - D) {
    static_for<0, S>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      const int t = lane * S + j - (64 * S - H);
      if (t >= 0) lds.tail[q][t] = z[j];
    });
  }
  __syncthreads();                                                      // ---- A
  // offsets of this wave and of the wave below it: totals of the waves below, ascending
  double woff = 0.0, woff_below = 0.0;
  {
    double run = 0.0;
#pragma unroll
    for (int k = 0; k + 1 < SPLIT_WAVES; ++k) {
      if (q == k + 1) woff_below = run;
      run += lds.tail[k][H - 1];
      if (q == k + 1) woff = run;
    }
  }
#pragma unroll
  for (int j = 0; j < S; ++j) z[j] += woff;
  double Z[H + S];
  exact_window_below<S, KT>(z, Z);
  if (q > 0 && lane < D) {                 // the DPP shifts ran off the wave: the tail of the wave below, offset as its owner does
    static_for<0, H>([&](auto ec) {
      constexpr int e = decltype(ec)::value;
      const int t = lane * S + e;
      if (t < H) Z[e] = lds.tail[q - 1][t] + woff_below;
    });
  }
  exact_fir_residual<S, KT>(Z, y, mk, taps, r);
  if (lane < D) {
    static_for<0, S>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      const int t = lane * S + j;
      if (t < H) lds.head[q][t] = r[j];
    });
  }
}

// backward half (behind barrier B): g = revcumsum(K^T r) over the whole series, gradient step, prox, momentum; with a stop
// rule the two sums of its criterion over the WHOLE series come back in num / den, the same bits in every wave.  Holds
// barrier C and, with a stop rule, D.
template <int S, int KT, int STOP, class TAPS>
__device__ __forceinline__ void split_backward(const double (&r)[S], double (&w)[S], const TAPS& taps, double nstep,
                                               double th, const double* beta_k, double (&uprev)[STOP == 2 ? S : 1],
                                               double (&d1)[STOP == 2 ? S : 1], double (&d2)[STOP == 2 ? S : 1],
                                               double (&d3)[STOP == 2 ? S : 1], double& num, double& den, SplitLds<KT>& lds,
                                               int q, int lane) {
  constexpr int H = KT - 1;
  constexpr int D = (H + S - 1) / S;
  double R[S + H];
  exact_window_above<S, KT>(r, R);
  if (q + 1 < SPLIT_WAVES && lane >= 64 - D) {      // past the wave's last lane: the head of the wave above
    static_for<S, S + H>([&](auto ec) {
      constexpr int e = decltype(ec)::value;
      const int t = lane * S + e - 64 * S;
      if (t >= 0) R[e] = lds.head[q + 1][t];
    });
  }
  double g[S];
  exact_corr_suffix<S, KT>(R, taps, g);
  double off = wave_suffix_excl_f64(g[0]);          // sum of the lanes above within the wave
  if (lane == 0) lds.gtot[q] = g[0] + off;          // the wave's total
  __syncthreads();                                                      // ---- C
  {
    double run = 0.0, above = 0.0;
#pragma unroll
    for (int k = SPLIT_WAVES - 1; k >= 1; --k) {
      run += lds.gtot[k];
      if (q == k - 1) above = run;
    }
    off += above;                                   // additions only: exactly 0 above the last sample
  }
#pragma unroll
  for (int j = 0; j < S; ++j) g[j] += off;

  exact_update<S, STOP>(g, w, nstep, th, beta_k, uprev, d1, d2, d3, num, den);
  if constexpr (STOP != 0) {
    num = seg_allsum_f64<64>(num);
    den = seg_allsum_f64<64>(den);
    if (lane == 0) {
      lds.num[q] = num;
      lds.den[q] = den;
    }
    __syncthreads();                                                    // ---- D
    num = (lds.num[0] + lds.num[1]) + (lds.num[2] + lds.num[3]);
    den = (lds.den[0] + lds.den[1]) + (lds.den[2] + lds.den[3]);
  }
}

template <int S, int KT, bool WITH_J, int STOP>
__global__ __launch_bounds__(64 * SPLIT_WAVES) void fista_exact_split_kernel(FistaArgs a, TapsD<KT> taps) {
  static_assert(SPLIT_WAVES == 4, "the sums over the waves are written for four");
  __shared__ SplitLds<KT> lds;
  const int lane = threadIdx.x & 63;
  const int q = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // one slot of this launch's list per WORKGROUP (fista_fast.h: launch_slots): everything up to `live` is the same in its
  // four waves, so the workgroup of an empty candidate launch leaves as a whole
  int s0, s1;
  launch_slots(a, s0, s1);
  const int slot = (int)blockIdx.x + s0;
  if (slot >= s1 && a.range) return;
  bool live;
  const int p = slot_to_problem(a, slot, s1, live);
  const int base = (q * 64 + lane) * S;

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
int launch_exact_split(const FistaArgs& a, const double* taps, int K, bool with_j, int stop, hipStream_t st) {
  const auto td = make_taps_d<KT>(taps, K);
  const dim3 grid((unsigned)launch_count(a)), block(64 * SPLIT_WAVES);
  return launch_solve_variants(grid, block, with_j, stop, st, [&](auto wj, auto sm, dim3 g, dim3 b, hipStream_t s) {
    hipLaunchKernelGGL((fista_exact_split_kernel<S, KT, decltype(wj)::value, decltype(sm)::value>), g, b, 0, s, a, td);
  });
}

}  // namespace pb
