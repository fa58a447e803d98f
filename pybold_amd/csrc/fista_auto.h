// The noise-driven lambda search of deconv (lbda=None, pybold/bold_signal.py:99-214) as ONE device-resident solve:
// one voxel per wave64, carried through  inner solve -> residual -> alpha update -> alpha window  until that voxel is
// done.  Nothing of the search depends on another voxel, so nothing goes back to the host between outer iterations
// (the host loop of pybold_amd/bold_signal.py::_deconv_auto_lbda re-solves every voxel, stopped ones included, with
// two launches, two device->host copies and a sync per outer iteration).
//
// The inner solve is the pass body of fista_exact_kernel<S, KT, false, 2> (fista_exact.h: exact_forward /
// exact_backward, shared, not copied): float64 end to end, y, w, the mask and the window-rule state in VGPRs, the
// reference's prox for a NEGATIVE threshold (prox_excess_ref) and the additions-only suffix scan -- lambda does go
// negative in the reference's own runs.  Per outer iteration i (the branch as the repository's NumPy checker restates it):
//   inner solve   warm-started from w, momentum restarted (betas[0..]), at most nb_sub_iter iterations, threshold
//                 lbda * step; STOP == 2: the window rule (wind = 6, first test at it >= 7, floor 3e-10, state zeroed at
//                 the start of every inner solve); STOP == 0 (early_stopping off): all nb_sub_iter iterations      :114-138
//   statistics    r = sum (h * cumsum(w) - y)^2, g = sum |w| from the forward pass that follows the last update      :141, :150-153
//   alpha         alpha += mu (r - N sigma^2), mu = 1e-4; lbda = 1 / (2 alpha); J_i = 0.5 r + lbda g (updated lbda),
//                 NOT contracted to FMAs: the host loop's NumPy lines are not                                       :141-157
//   alpha window  STOP == 2 and i > 6: old = mean(alpha_{i-5..i-3}), new = mean(alpha_{i-2..i}); the voxel stops when
//                 |new - old| / |new| < tol, keeping its iterate and its lambda                                     :164-178
// and after the loop one more inner solve with the last lambda (:181-209).
//
// RESUMABLE: a voxel may need nb_iter * nb_sub_iter = 1e6 inner iterations, so a launch runs the outer iterations
// [i0, i1) of the voxels that are not done (a wave whose voxel is done leaves at once) and the state of the search
// -- alpha, lbda, the ring of the last six alphas, the outer index, the done flag, the inner-iteration count -- lives
// between launches in AUTO_STATE float64 slots per voxel beside w.  Everything that crosses a launch boundary is a
// float64 / integer stored and reloaded as is, and every inner solve starts from zeroed window state whether or not a
// launch boundary precedes it: the chunking changes no bit of any output.
#pragma once
#include "fista_exact.h"

namespace pb {

constexpr int AUTO_STATE = 12;      // float64 slots per voxel: alpha, lbda, ring[6], outer index, done, n_inner, (spare)
constexpr int AUTO_WIND = 6;

struct AutoArgs {
  const double* y;                  // [V][ldy]
  int64_t ldy;
  double* w;                        // [V][ldw]: iterate between launches, final iterate
  int64_t ldw;
  int V, N;
  int cold;                         // first launch only: start from w = 0 instead of reading w
  int init;                         // first launch: the state starts at alpha = 1, lbda = 1/2
  int i0, i1;                       // outer iterations of this launch
  int final_solve;                  // after them: the last inner solve, then the outputs
  int nb_sub_iter;
  double step, tol;
  const double* betas;              // [nb_sub_iter]
  const double* sigma;              // [V]
  double *R, *G, *J;                // [V][ldt] traces or nullptr
  int64_t ldt;
  double *alpha_out, *lbda_out;     // [V]
  int32_t* n_outer;                 // [V]
  int64_t* n_inner;                 // [V]
  double* work;                     // [V][AUTO_STATE]
};

// :141-157 as NumPy evaluates it: every product and sum rounded on its own
__device__ __forceinline__ void auto_alpha_update(double r, double g, double n_sigma2, double& alpha, double& lbda, double& cost) {
#pragma clang fp contract(off)
  const double grad = r - n_sigma2;
  alpha = alpha + 1.0e-4 * grad;
  lbda = 1.0 / (2.0 * alpha);
  cost = 0.5 * r + lbda * g;
}

// :164-178 on the ring of the last six alphas (oldest first): np.mean adds in order, then divides
__device__ __forceinline__ bool auto_alpha_window_fires(const double (&ring)[AUTO_WIND], double tol) {
#pragma clang fp contract(off)
  const double older = ((ring[0] + ring[1]) + ring[2]) / 3.0;
  const double newer = ((ring[3] + ring[4]) + ring[5]) / 3.0;
  return fabs(newer - older) / fabs(newer) < tol;
}

__device__ __forceinline__ double auto_n_sigma2(int N, double sigma) {
#pragma clang fp contract(off)
  return (double)N * (sigma * sigma);
}

template <int S, int KT, int STOP>
__global__ __launch_bounds__(256) void auto_lbda_kernel(AutoArgs a, TapsD<KT> taps) {
  static_assert(STOP == 0 || STOP == 2, "the search stops its inner solves on the window rule or not at all");
  const int lane = threadIdx.x & 63;
  const int v = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
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
    // ---- inner solve from w with the current lambda; leaves r = the residual of its last iterate ----
    if constexpr (STOP == 2) {
#pragma unroll
      for (int j = 0; j < S; ++j) uprev[j] = d1[j] = d2[j] = d3[j] = 0.0;
    }
    const double th = lbda * a.step;
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
int launch_auto(const AutoArgs& a, const double* taps, int K, bool early_stopping, hipStream_t st) {
  const auto td = make_taps_d<KT>(taps, K);
  const dim3 grid((unsigned)((a.V + 3) / 4)), block(256);
  if (early_stopping) hipLaunchKernelGGL((auto_lbda_kernel<S, KT, 2>), grid, block, 0, st, a, td);
  else hipLaunchKernelGGL((auto_lbda_kernel<S, KT, 0>), grid, block, 0, st, a, td);
  return 0;
}

}  // namespace pb
