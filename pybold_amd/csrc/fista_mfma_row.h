// One series per WAVE on the matrix pipe: the plain FISTA solve for the few dense rows that the whole rounds of the
// one-wave form (fista_mfma.h, fista_mfma_sparse.h: 16 problems per wave) leave behind, and for any batch small enough to
// run one series per wave.
//
// The forms that put 16 problems into a wave chain the blocks of a series one after the other; one pass of them costs a
// whole round however few problems there are.  Here the 16 columns of a 16x16x32 product are the 16 BLOCKS of one series
// (32 samples each, up to 512 scans), so every block of a pass is computed at once and nothing is chained:
//
//   x_n = C0 w_n + C1 w_{n-1} + S sum_{b <= n-2} sum(w_b)            c = 2^a cumsum(h) (MfmaTaps), S = c[K-1], K <= 33
//   g_n = C0^T r_n + C1^T r_{n+1} + S sum_{b >= n+2} sum(r_b)        r = x - y
//
// C0 / C1 are the two dense near tiles (lags ko - ki and 32 + ko - ki); the operand of C1 is the wave's own operand moved one
// lane up inside its row of 16 (DPP row_shr:1 on the eight packed words, zero into column 0), the adjoint's one lane down.
// The far field is constant (lag >= 33 >= K-1): a per-block sum over the four lanes of a column, a prefix (suffix) sum over
// the 16 lanes of a row and eight v_fma_f32 per lane, all float32, from the unsplit values.  24 matrix instructions and
// about 150 vector instructions per iteration.
//
// Mapping: lane (n = lane & 15, g = lane >> 4) holds samples t = 32 n + 8 g + j, j < 8 -- the B-operand layout of the
// instruction, and with the tile rows permuted as in fista_mfma.h (row 4 g + i of row half r <-> slot 8 g + 4 r + i) its D
// layout too: operands, accumulators and the float64 iterate of a sample share a lane, the update works in place.
//
// Arithmetic: that of the other matrix-pipe forms (mfma_core.h): split_pair for iterate and residual, split8 for the tiles,
// three products per tile, float32 accumulation, float64 iterate and update, the same series scale and g_scale.
// Hand-back: the range guard runs EVERY iteration (eight samples per lane: two v_max3_f32 per four samples) and is sticky: a
// row whose |sigma w| reached 60000 or whose residual reached 2^15 at any iteration, a degenerate row, and under rho_guard a
// row with th > MFMA_RHO_MAX max|sigma w| is not stored and gets n_done = -1.  The in-loop maxima are float maxima, which
// drop a NaN: a non-finite iterate is caught AT THE STORE instead, where iterate_absmax ranks the final iterate by its bits
// (NaN and inf highest) -- a NaN, once in w, stays there through every later update, so nothing is missed by waiting.
// Plain solves only: taps from the host, no cost trace, no stop rule, no only_flagged pass.
#pragma once
#include "mfma_core.h"

namespace pb {

constexpr int ROW_NMIN = 129, ROW_NMAX = 320, ROW_KMAX = 33;      // what is dispatched (the mapping itself holds 512 scans)

// one series per wave, four waves per workgroup; 0: launched, 1: not this kernel's shape (defined in mfma_row_inst.hip)
int launch_mfma_row(const FistaArgs& a, const double* taps, int K, bool with_j, hipStream_t st);

#ifdef PB_MFMA_ROW_INST                          // (the kernel is no template: it is compiled in its own object only)

__device__ __forceinline__ unsigned row_word_from_below(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, DPP_ROW_SHR + 1, 0xf, 0xf, true);
}
__device__ __forceinline__ unsigned row_word_from_above(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, DPP_ROW_SHL + 1, 0xf, 0xf, true);
}
template <bool UP>
__device__ __forceinline__ Frag row_neighbour(const u4& h, const u4& l) {
  u4 nh, nl;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    nh[c] = UP ? row_word_from_below(h[c]) : row_word_from_above(h[c]);
    nl[c] = UP ? row_word_from_below(l[c]) : row_word_from_above(l[c]);
  }
  return Frag{__builtin_bit_cast(h8, nh), __builtin_bit_cast(h8, nl)};
}
// a value of each of a column's four lanes (n, n + 16, n + 32, n + 48) -> their sum, the same bits in every one of them.
// Two register swaps (v_permlane32_swap: the upper half of the first operand against the lower half of the second;
// v_permlane16_swap: its odd rows of 16 against the even rows of the second) and two additions: the shuffles of group_sum
// go through LDS and make their addresses in the loop (a dozen vector instructions per sum where registers are short).
// (Inline assembly, the two wait states a swap needs behind a vector write of its operands inside the string.  With the
// builtins __builtin_amdgcn_permlane32_swap / _permlane16_swap, both arguments the same value, this kernel's listing added
// the FIRST result to itself and the far field came out wrong -- the listing lines, the compiler's version and the failing
// figures: profiles/mfma_leftovers_ab.txt, section 6.  Whether the builtins are at fault with two different values was not
// tried.)
__device__ __forceinline__ float column_sum(float x) {
  float a = x, b = x;
  asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));       // (lanes l and l ^ 32 side by side)
  a += b;
  b = a;
  asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));       // (rows 2 k and 2 k + 1 side by side)
  return a + b;
}
// (the lane index is the caller's: the epilogue passes a laundered one, so that no shuffle address of the prologue is kept
// -- spilled, as it was -- through the solve)
__device__ __forceinline__ float wave_max(float x, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1)
    x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((lane ^ o) << 2, __builtin_bit_cast(int, x))));
  return x;
}

// Four waves per workgroup, no workgroup barrier: the waves share nothing.  (With ONE wave per workgroup, 10 of the 28
// launches behind the main kernel in a kernel trace of the benchmark took 0.57 ms, the other 18 0.41 ms; with four, all 29
// took 0.39 -- profiles/mfma_leftovers_ab.txt, section 5.  That the slow launches had three waves on some SIMD is a
// supposition: no counter was read.)  At most 128 registers: four waves per SIMD.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void fista_mfma_row_kernel(FistaArgs a, MfmaTaps tp) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n = lane & 15, g = lane >> 4;
  int s0 = 0, n_list = 0;                        // this launch's slots [s0, n_list) of its list
  launch_slots(a, s0, n_list);
  const int slot = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + wv) + s0;
  if (slot >= n_list) return;                    // (the same in every lane of the wave: a scalar branch)
  bool live;
  const int p = __builtin_amdgcn_readfirstlane(slot_to_problem(a, slot, n_list, live));

  __shared__ float lc_wg[4][64];                 // cumulative taps, lags 0 .. 63 (a copy per wave: no workgroup barrier)
  __shared__ f4 lys_wg[4][2][64];                // -2^a sigma y: read back once per iteration as the accumulators' start
  float* lc = lc_wg[wv];
  f4 (*lys)[64] = lys_wg[wv];
  lc[lane] = tp.c[lane];
  wave_sync();
  const float sfar = lc[63];

  // ---- load the series, scale it into the float16 range (the scale of fista_mfma.h) ----
  const int t0 = 32 * n + 8 * g;
  const double lb = a.lbda_vec ? a.lbda_vec[p] : a.lbda;
  float ysn[8];                                  // -2^a sigma y
  double w[1][8];                                // sigma w
  float sigma = 1.0f, inv_sigma = 1.0f;
  bool degenerate = false;
  {
    const float* yrow = a.y + (int64_t)(p / a.y_rep) * a.ldy;
    float m = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int t = t0 + j;
      float yl = yrow[t < a.N ? t : a.N - 1];    // (clamped address + select: no exec-masked region)
      ysn[j] = t < a.N ? yl : 0.0f;
      m = fmaxf(m, fabsf(ysn[j]));
    }
    m = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, wave_max(m, lane))));
    const bool okm = m > 0.0f && m < 3.0e38f;
    int e = 0;
    (void)frexpf(okm ? m : 1.0f, &e);
    e = __builtin_amdgcn_readfirstlane(e);       // (the scale is the wave's: scalar registers hold it through the solve)
    const float sg = ldexpf(1.0f, a.ybits - e) / tp.y_scale, isg = ldexpf(1.0f, e - a.ybits) * tp.y_scale;
    sigma = okm ? sg : 1.0f;
    inv_sigma = okm ? isg : 1.0f;
    degenerate = !okm && !a.cold;
    const float ys = -sigma * tp.y_scale;
    const double* wrow = a.w + (int64_t)p * a.ldw;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      ysn[j] *= ys;
      w[0][j] = 0.0;
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) lys[r][lane] = f4{ysn[4 * r], ysn[4 * r + 1], ysn[4 * r + 2], ysn[4 * r + 3]};
    if (!a.cold) {                               // (the same for every lane: a scalar branch)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int t = t0 + j;
        const double wl = wrow[t < a.N ? t : a.N - 1] * (double)sigma;
        w[0][j] = t < a.N ? wl : 0.0;
      }
    }
  }
  const double th = lb * a.step * (double)sigma;
  const double nstep = -a.step * tp.g_scale;
  const int nvalid = a.N - t0;                   // samples j < nvalid of this lane are real
  // ---- operator tiles (A operands): lane holds row rho = lane & 15, k = 8 (lane >> 4) + j ----
  // (built AFTER the series is loaded, one pair at a time: with the tiles live across the loads, or all in flight at once,
  // the compiler spilled 16 registers to scratch in this prologue)
  __builtin_amdgcn_sched_barrier(0);
  Frag An[2][2], Bn[2][2];                       // forward near [r][o], adjoint near [r][o]
  {
    const int rho = lane & 15, kg = lane >> 4, gp = rho >> 2, i = rho & 3;
    auto cval = [&](int lag) -> float {            // (branch-free: clamped address + select)
      const float c = lc[lag < 0 ? 0 : (lag > 63 ? 63 : lag)];
      return lag < 0 ? 0.0f : c;
    };
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int o = 0; o < 2; ++o) {
        float fa[8], fb[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int ko = 8 * gp + 4 * r + i, ki = 8 * kg + j;
          fa[j] = cval(32 * o + ko - ki);
          fb[j] = cval(32 * o + ki - ko);
        }
        An[r][o] = split8(fa);
        Bn[r][o] = split8(fb);
        __builtin_amdgcn_sched_barrier(0);
      }
  }

  float wmax = 0.0f, rmax = 0.0f;                // sticky: largest |sigma w| and |residual| any iteration saw
  double dummy0 = 0.0, dummy1 = 0.0;

  for (int it = 0; it < a.n_iter; ++it) {
    const double nb1 = -(1.0 + a.betas[it]);
    // ---- forward: r = T_c w - y ----
    float x[8];
    u4 ph, pl;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      x[j] = (float)w[0][j];
      wmax = fmaxf(wmax, fabsf(x[j]));
    }
#pragma unroll
    for (int pp = 0; pp < 4; ++pp) {
      unsigned h2, l2;
      (void)split_pair(x[2 * pp], x[2 * pp + 1], h2, l2);
      ph[pp] = h2;
      pl[pp] = l2;
    }
    // far field: S (sum of the blocks up to n-2), float32, from the unsplit iterate
    const float fsum = column_sum(((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7])));
    const Frag wf{__builtin_bit_cast(h8, ph), __builtin_bit_cast(h8, pl)};
    const Frag wf1 = row_neighbour<true>(ph, pl);                  // block n-1
    f4 acc[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) acc[r] = lys[r][lane];           // (each lane reads what it wrote: no barrier)
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int r = 0; r < 2; ++r) acc[r] = mfma_part(An[r][0], wf, acc[r], k);
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int r = 0; r < 2; ++r) acc[r] = mfma_part(An[r][1], wf1, acc[r], k);
    {
      const float far = sfar * row_from_below<2>(row_prefix_incl(fsum));
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float rj = acc[j >> 2][j & 3] + far;
        x[j] = j < nvalid ? rj : 0.0f;             // padding behind sample N-1 carries no residual
        rmax = fmaxf(rmax, fabsf(x[j]));
      }
    }
    // ---- adjoint: g = T_c^T r ----
#pragma unroll
    for (int pp = 0; pp < 4; ++pp) {
      unsigned h2, l2;
      (void)split_pair(x[2 * pp], x[2 * pp + 1], h2, l2);
      ph[pp] = h2;
      pl[pp] = l2;
    }
    const float bsum = column_sum(((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7])));
    const Frag rf{__builtin_bit_cast(h8, ph), __builtin_bit_cast(h8, pl)};
    const Frag rf1 = row_neighbour<false>(ph, pl);                 // block n+1
#pragma unroll
    for (int r = 0; r < 2; ++r) acc[r] = mfma_part(Bn[r][0], rf, f4{0.f, 0.f, 0.f, 0.f}, 0);
#pragma unroll
    for (int k = 1; k < 3; ++k)
#pragma unroll
      for (int r = 0; r < 2; ++r) acc[r] = mfma_part(Bn[r][0], rf, acc[r], k);
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int r = 0; r < 2; ++r) acc[r] = mfma_part(Bn[r][1], rf1, acc[r], k);
    {
      const float far = sfar * row_from_above<2>(row_suffix_incl(bsum));
      // ---- update (float64, in place) ----
#pragma unroll
      for (int j = 0; j < 8; ++j)
        (void)fista_update<false>(w[0][j], acc[j >> 2][j & 3] + far, nstep, th, nb1, dummy0, dummy1);
    }
  }

  // ---- store (unscaled); a row that came near the float16 range, or too sparse a one, is handed back ----
  int le = threadIdx.x & 63;
  asm volatile("" : "+v"(le));
  const float wlast = wave_max(iterate_absmax<1>(w), le);
  const float guard = wave_max(fmaxf(fmaxf(wmax, wlast), rmax >= 32768.0f ? 65504.0f : 0.0f), le);
  const bool bad = !(guard < 60000.0f) || degenerate || (a.rho_guard && wlast > 0.0f && (float)th > MFMA_RHO_MAX * wlast);
  if (live && !bad) {
    // (the lane's first sample made HERE again, from the laundered lane index)
    const int te = 32 * (le & 15) + 8 * (le >> 4);
    double* wrow = a.w + (int64_t)p * a.ldw + te;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (te + j < a.N) wrow[j] = w[0][j] * (double)inv_sigma;
  }
  if (live && a.n_done && lane == 0) a.n_done[p] = bad ? -1 : a.n_iter;
}

int launch_mfma_row(const FistaArgs& a, const double* taps, int K, bool with_j, hipStream_t st) {
  if (a.N < ROW_NMIN || a.N > ROW_NMAX || K < 1 || K > ROW_KMAX) return 1;
  if (with_j || a.stop_mode != 0 || a.taps_pp || a.only_flagged || !taps) return 1;
  const int64_t waves = launch_count(a);
  if (waves <= 0) return 0;
  const MfmaTaps tp = make_mfma_taps(taps, K);
  hipLaunchKernelGGL(fista_mfma_row_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, a, tp);
  return 0;
}
#endif

}  // namespace pb
