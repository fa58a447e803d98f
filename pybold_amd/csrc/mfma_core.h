// What the three matrix-pipe FISTA kernels state alike: fista_mfma_kernel (fista_mfma.h, one wave per 16 problems),
// mfma2_role (fista_mfma2.h, a series over two waves) and mfma4_role (fista_mfma4.h, over four).  Types, the float16
// split, the barriers, the lane-group reductions, the float64 update, the
// window rule's certificate, the two halves of the range guard and the _loops_deconv criterion live here, once, each
// with the code-generation rule that protects it.  The kernel files keep what is theirs: the block layout (31 samples +
// sum slot, or 32 samples + carry tile), the hand-pipelined slot order of the two passes, the LDS layout, the exchange
// between waves, the loads and stores.
//
// These kernels are scheduled by hand at the grain of single matrix instructions and several sit at the edge of the
// register file, so a helper is here only if every dispatched variant compiles to the SAME registers, scratch, LDS and
// matrix / LDS / memory instruction counts with it as without (tools/isa_diff.py against a build of the commit before;
// profiles/mfma_core_isa.txt).  What did not pass stays in the kernels, restated, and DESIGN 5 says what and why.  The
// shapes that pass: __forceinline__, values in and out or references to single scalars; NOT a struct returned by value
// that a kernel then spreads over its own variables, and not the guards by reference next to the iterate array.
#pragma once
#include "../../include/pybold_hip.h"
#include "common.h"
#include "fista_fast.h"

namespace pb {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned u4 __attribute__((ext_vector_type(4)));
typedef unsigned u3 __attribute__((ext_vector_type(3)));

constexpr float MFMA_RHO_MAX = 0.02f;

struct MfmaTaps {
  float c[96];      // 2^a * cumsum(h)[m], m < 96 (constant from m = K-1 on; K <= 33 uses 64 of them)
  double g_scale;   // 2^(-2a): the gradient comes out scaled by 2^(2a)
  float y_scale;    // 2^a
};

inline MfmaTaps make_mfma_taps(const double* taps, int K) {
  MfmaTaps t;
  double c[96], run = 0.0, cmax = 0.0;
  for (int m = 0; m < 96; ++m) {
    if (m < K) run += (double)(float)taps[m];
    c[m] = run;
    cmax = fabs(run) > cmax ? fabs(run) : cmax;
  }
  int e = 0;
  if (cmax > 0.0) frexp(cmax, &e);          // cmax = f 2^e, f in [0.5, 1)
  const int a = 3 - e;                       // max |c| 2^a in [4, 8)
  for (int m = 0; m < 96; ++m) t.c[m] = (float)ldexp(c[m], a);
  t.g_scale = ldexp(1.0, -2 * a);
  t.y_scale = (float)ldexp(1.0, a);
  return t;
}

struct Frag {
  h8 hi, lo;
};

typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef float f2v __attribute__((ext_vector_type(2)));
// two float32 -> packed float16, round to nearest even (v_cvt_pk_f16_f32).  The LOW parts are
// rounded, not truncated: a truncated split shrinks every operand by ~2^-23 on average, a bias
// that adds up coherently over samples and iterations (measured: 14x the error of float32
// operators along a regularisation path, tools/r3_mfma_precision.py).
__device__ __forceinline__ unsigned pk_rne(float x0, float x1) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f2v{x0, x1}, h2));
}

// (x0, x1) -> packed hi = RTZ(x) and packed lo = RNE(x - hi); x - hi is exact in float32.  Returns x1 - hi(x1), the
// difference before its rounding (split_pair_rem goes on from it).
// (v_fma_mixlo_f16 + v_fma_mixhi_f16 would write the rounded differences straight into the two
// halves -- one instruction less per pair, 96 fewer per iteration -- and measured 4.5 % SLOWER:
// profiles/r3_mfma_split_mixlo_ab.txt; the partial-register writes serialise.)
__device__ __forceinline__ float split_pair(float x0, float x1, unsigned& hi, unsigned& lo) {
  hi = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(x0, x1));
  float l0, l1;
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(l0) : "v"(hi), "v"(x0));
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(l1) : "v"(hi), "v"(x1));
  lo = pk_rne(l0, l1);
  return l1;
}

// split_pair, and what the split drops of x1: rem = x1 - hi - lo (exact)
__device__ __forceinline__ void split_pair_rem(float x0, float x1, unsigned& hi, unsigned& lo, float& rem) {
  const float l1 = split_pair(x0, x1, hi, lo);
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(rem) : "v"(lo), "v"(l1));
}

// eight float32 -> float16 hi / lo parts (hi = RTZ(x), lo = RNE(x - hi): 22 bits, unbiased)
__device__ __forceinline__ Frag split8(const float (&x)[8]) {
  u4 ph, pl;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    unsigned h2, l2;
    (void)split_pair(x[2 * p], x[2 * p + 1], h2, l2);
    ph[p] = h2;
    pl[p] = l2;
  }
  return Frag{__builtin_bit_cast(h8, ph), __builtin_bit_cast(h8, pl)};
}

// one of the three products of a split pair (acc += (Ahi + Alo) (Bhi + Blo) without the lo.lo term): hi.hi, hi.lo, lo.hi
__device__ __forceinline__ f4 mfma_part(const Frag& A, const Frag& B, f4 acc, int part) {
  return part == 0   ? __builtin_amdgcn_mfma_f32_16x16x32_f16(A.hi, B.hi, acc, 0, 0, 0)
         : part == 1 ? __builtin_amdgcn_mfma_f32_16x16x32_f16(A.hi, B.lo, acc, 0, 0, 0)
                     : __builtin_amdgcn_mfma_f32_16x16x32_f16(A.lo, B.hi, acc, 0, 0, 0);
}

// the lanes of this wave: everything written to LDS before is visible after
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// every wave of the workgroup: everything written to LDS before is visible after
__device__ __forceinline__ void wg_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// a value of each of a problem's four lanes (v, v + 16, v + 32, v + 48) -> their maximum / sum, in every one of them
__device__ __forceinline__ float group_max(float x) {
  x = fmaxf(x, __shfl_xor(x, 16, 64));
  return fmaxf(x, __shfl_xor(x, 32, 64));
}
template <typename T>
__device__ __forceinline__ T group_sum(T x) {
  x += __shfl_xor(x, 16, 64);
  return x + __shfl_xor(x, 32, 64);
}
// (two sums at once, their shuffles interleaved: the second hides the latency of the first)
template <typename T>
__device__ __forceinline__ void group_sum2(T& x, T& y) {
  x += __shfl_xor(x, 16, 64);
  y += __shfl_xor(y, 16, 64);
  x += __shfl_xor(x, 32, 64);
  y += __shfl_xor(y, 32, 64);
}

// ---- range guard: the largest |sigma w| of this lane (NaN and inf rank highest: by the float32 bits) ... ----
template <int NBW>
__device__ __forceinline__ float iterate_absmax(const double (&w)[NBW][8]) {
  unsigned mb = 0;
#pragma unroll
  for (int q = 0; q < NBW; ++q)
#pragma unroll
    for (int j = 0; j < 8; ++j) mb = max(mb, __builtin_bit_cast(unsigned, (float)w[q][j]) & 0x7fffffffu);
  return mb >= 0x7f800000u ? 65504.0f : __builtin_bit_cast(float, mb);
}
// ... and whether a hi half of this lane's residual fragments (LDS copy) reached 2^15 (float16 bits of |hi|: 0x7800 = 32768)
template <int NBW>
__device__ __forceinline__ float residual_guard(const u4* lrf) {
  unsigned e = 0;
#pragma unroll
  for (int q = 0; q < NBW; ++q) {
    const u4 h = lrf[(2 * q) * 64];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      e = max(e, h[c] & 0x7fffu);
      e = max(e, (h[c] >> 16) & 0x7fffu);
    }
  }
  return e >= 0x7800u ? 65504.0f : 0.0f;
}
// ---- the window rule as a no-fire certificate (see fista_pair_ffa.h): constants and limits ----
constexpr float MFMA_CP1 = 0.3133f, MFMA_CP2 = 0.6467f, MFMA_CP3 = 0.04f;

// (1.001 tol)^2, and the limit the certificate's sum over a problem has to stay above (nblocks: blocks of the WHOLE series)
__device__ __forceinline__ float cert_tol2(double tol) { return ((float)tol * 1.001f) * ((float)tol * 1.001f); }
__device__ __forceinline__ float cert_limit(float cert_t2, double th, float sigma, int nblocks) {
  const float cert_c0 = (float)th * (4.0f * 1.0001f) * __builtin_sqrtf(32.0f * nblocks) + 3.1e-10f * sigma;
  return cert_t2 * cert_c0 * cert_c0 * (1.0001f / MFMA_CP3);
}

// ---- soft threshold + momentum of one sample: u = w - step g, d = clamp(u, +-th), w' = u - (1 + beta) d ----
// LOOPS: d and w' also enter this lane's parts of ||d||^2 and ||w'||^2 (the _loops_deconv rule; the caller alternates two
// accumulators of each by sample parity).  Returns u (the certificate tracks it).
template <bool LOOPS>
__device__ __forceinline__ double fista_update(double& w, float g, double nstep, double th, double nb1, double& dsq, double& wsq) {
  const double u = fma(nstep, (double)g, w);
  const double d = fmin(fmax(u, -th), th);
  w = fma(nb1, d, u);
  if constexpr (LOOPS) {
    dsq = fma(d, d, dsq);
    wsq = fma(w, w, wsq);
  }
  return u;
}

// ---- the window rule's certificate (see fista_pair_ffa.h) ----
// Per-lane state in LDS, STRIDE floats apart: lt[0..3] ring of the tracked sample's last four increments, [4,5] its u_{k-1}
// (float64 halves), [6] this lane's ||w_k||^2 part.  The window combination on the tracked sample (u_k = cu, w_{k+1} = cw)
// of iteration cert_it: float32 from float64 differences; its rounding, and that of the stored increments, is below
// 2^-21 M.  Returns v^2 and moves the ring on.
template <int STRIDE>
__device__ __forceinline__ float cert_window(float* lt, int cert_it, double cu, double cw) {
  const float d1 = lt[((cert_it + 3) & 3) * STRIDE], d2 = lt[((cert_it + 2) & 3) * STRIDE], d3 = lt[((cert_it + 1) & 3) * STRIDE];
  const unsigned ulo = __builtin_bit_cast(unsigned, lt[4 * STRIDE]), uhi = __builtin_bit_cast(unsigned, lt[5 * STRIDE]);
  const double up = __builtin_bit_cast(double, ((unsigned long long)uhi << 32) | ulo);
  const float dk = (float)(cu - up), e = (float)(cw - cu);
  const float v = fmaf(2.0f, d2, fmaf(3.0f, d1, fmaf(2.0f, dk, e))) + d3;
  const float m = fmaf(2.0f, fabsf(d2), fmaf(3.0f, fabsf(d1), fmaf(2.0f, fabsf(dk), fabsf(e)))) + fabsf(d3);
  const float vs = fmaxf(fmaf(-0x1p-21f, m, fabsf(v)), 0.0f);
  lt[(cert_it & 3) * STRIDE] = dk;
  const unsigned long long ub = __builtin_bit_cast(unsigned long long, cu);
  lt[4 * STRIDE] = __builtin_bit_cast(float, (unsigned)ub);
  lt[5 * STRIDE] = __builtin_bit_cast(float, (unsigned)(ub >> 32));
  return vs * vs;
}

// this wave's part of  sum v^2 - tol^2 (||w_k||^2 / p1 + 4 ||w_{k+1}||^2 / p2)  over a problem's lanes (the rule is first
// tested at wind + 1 = 7; the certificate holds while the sum over the whole series stays >= cert_lim); stores ||w_{k+1}||^2
template <int STRIDE>
__device__ __forceinline__ float cert_term(float* lt, float cvsq, float cert_t2, float jw2) {
  const float t = group_sum(cvsq - cert_t2 * ((1.0001f / MFMA_CP1) * lt[6 * STRIDE] + (4.0001f / MFMA_CP2) * jw2));
  lt[6 * STRIDE] = jw2;
  return t;
}

// ---- the _loops_deconv criterion ||w' - u|| / (||w'|| + 1e-10) with ||w' - u|| = (1 + beta) ||d|| ----
// Everything lives at the scale sigma, and so does the reference's 1e-10 floor.  Evaluated in EVERY lane and pinned: under
// `lactive &&` the compiler evaluated it in an exec-masked region and parked live registers in accumulator registers
// there -- the pattern tools/isa_spill_lint.py refuses.
__device__ __forceinline__ double loops_criterion(double beta, double num, double den, float sigma) {
  double crit = (1.0 + beta) * sqrt(num) / (sqrt(den) + 1.0e-10 * (double)sigma);
  asm volatile("" : "+v"(crit));
  return crit;
}

}  // namespace pb
