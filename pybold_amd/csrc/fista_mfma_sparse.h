// The plain one-wave matrix-pipe FISTA solve (fista_mfma.h: 16 problems per wave, 31 samples + sum slot per block, K <= 32
// taps, no cost trace, no stop rule; taps from the host or shared in device memory) with BOTH near tiles of a block in one 2:4-sparse product:
// v_smfmac_f32_16x16x64_f16, 6 matrix instructions per block and pass instead of 12 (120 per iteration at 300 scans
// instead of 228).  The form x_q = C0 w_q - E w_{q-1} + S sum_{b <= q-1} w_b, why its joined row is 2:4 and the column
// order of the operands are in mfma_sparse_tiles.h; mapping, scales, the float64 update, the guards, the hand-back and the
// store are those of fista_mfma_kernel and stated there.
//
// Operands.  A pass keeps ONE B operand per split part: 8 registers, register 2t + e = pair t of the block of parity e.
// Block q+1 overwrites the words of block q-1 only, so a fragment is written once and is "own" for its block's products
// and "other" for the next block's.  No word of a tuple may be written while a product still ahead in program order
// reads the tuple: the next block's hi words (v_cvt_pkrtz) come behind this block's last product, its lo words
// (v_cvt_pk_f16) too; the first and the last block of a pass find zeros in the other parity's words.
// Product order per block: the row half with the sum row first (its result feeds the next block's sum slot), per row
// half hi.hi, A.hi B.lo, A.lo B.hi.  The wait for the sum row is filled with the neighbours' vector work: residual
// fragments of the block before (forward), float64 updates of the block behind (adjoint).
#pragma once
#include "fista_mfma.h"
#include "mfma_sparse_tiles.h"

namespace pb {

typedef _Float16 h16 __attribute__((ext_vector_type(16)));
typedef unsigned u8 __attribute__((ext_vector_type(8)));

// one of the three products of a split pair with a sparse A tile: hi.hi, hi.lo, lo.hi
__device__ __forceinline__ f4 smfmac_part(const Frag& A, int idx, const u8& bh, const u8& bl, f4 acc, int part) {
  return part == 0   ? __builtin_amdgcn_smfmac_f32_16x16x64_f16(A.hi, __builtin_bit_cast(h16, bh), acc, idx, 0, 0)
         : part == 1 ? __builtin_amdgcn_smfmac_f32_16x16x64_f16(A.hi, __builtin_bit_cast(h16, bl), acc, idx, 0, 0)
                     : __builtin_amdgcn_smfmac_f32_16x16x64_f16(A.lo, __builtin_bit_cast(h16, bh), acc, idx, 0, 0);
}

// TAPS_DEV: the HRF and the step are read from device memory (a.taps_pp: K float64 shared by every problem,
// a.step_vec[0]), as in fista_mfma_kernel: the shared-HRF z-step computes what the host-taps solve computes, bit for bit.
// GROUPED: one HRF and one step per parcel, a wave's problems from the unit table -- fista_mfma_kernel's GROUPED, restated.
template <int NB, bool TAPS_DEV = false, bool GROUPED = false>
__global__ __launch_bounds__(256) void fista_mfma_sparse_kernel(FistaArgs a, MfmaTaps tp) {
  static_assert(!GROUPED || TAPS_DEV, "parcels take their taps from device memory");
  const int lane = threadIdx.x & 63;
  const int v = lane & 15, g = lane >> 4;
  const int wave = (int)((blockIdx.x * 256 + threadIdx.x) >> 6);
  int s0 = 0, n_list = 0;
  if constexpr (!GROUPED) {
  launch_slots(a, s0, n_list);
  if (__builtin_amdgcn_readfirstlane(wave) * 16 + s0 >= n_list) return;      // (a scalar branch, as in fista_mfma_kernel)
  } else {
    if (__builtin_amdgcn_readfirstlane(wave) >= *a.n_dense) return;
  }
  bool live;
  int parcel = 0;
  const int p = GROUPED ? grouped_problem(a, wave, v, live, parcel) : slot_to_problem(a, wave * 16 + v + s0, n_list, live);
  const int tb = 8 * g;
  const bool g3 = g == 3;

  extern __shared__ __attribute__((aligned(16))) char mf_smem[];
  u4* lrf = reinterpret_cast<u4*>(mf_smem) + ((threadIdx.x >> 6) * NB * 2 * 64 + lane);
  float* lc = reinterpret_cast<float*>(mf_smem + (size_t)4 * NB * 2 * 64 * sizeof(u4)) + (threadIdx.x >> 6) * 64;
  double step = a.step, g_scale = tp.g_scale;
  float y_scale = tp.y_scale;
  if constexpr (TAPS_DEV) {                       // (fista_mfma_kernel's prologue for two near tiles, restated)
    const double* taps_w = GROUPED ? a.taps_pp + (int64_t)parcel * a.ldt : a.taps_pp;
    double run = 0.0;
    for (int k = 0; k <= lane && k < a.K; ++k) run += (double)(float)taps_w[k];
    float cm = fabsf((float)run);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) cm = fmaxf(cm, __shfl_xor(cm, o, 64));
    int e = 0;
    if (cm > 0.0f) (void)frexpf(cm, &e);
    const int sa = 3 - e;
    lc[lane] = (float)ldexp(run, sa);
    g_scale = ldexp(1.0, -2 * sa);
    y_scale = ldexpf(1.0f, sa);
    step = a.step_vec[GROUPED ? parcel : 0];
  } else {
    lc[lane] = tp.c[lane];
  }
  wave_sync();

  // ---- operator tiles (sparse A operands) [pass][parity of the block][row half], and their position words ----
  Frag At[2][2][2];
  int ai[2][2][2];
  {
    auto cval = [&](int lag) -> float { return lag < 0 ? 0.0f : lc[lag > 63 ? 63 : lag]; };
#pragma unroll
    for (int ps = 0; ps < 2; ++ps)
#pragma unroll
      for (int par = 0; par < 2; ++par)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          float val[8];
          unsigned ix;
          (void)sparse_tile_lane(cval, ps, par, r, lane, val, ix);      // (K <= 32: the launcher's condition)
          At[ps][par][r] = split8(val);
          ai[ps][par][r] = (int)ix;
        }
  }

  // ---- load the problem, scale it into the float16 range (fista_mfma_kernel's prologue, restated) ----
  const double lb = a.lbda_vec ? a.lbda_vec[p] : a.lbda;
  float ysn[NB][8];                              // -2^a sigma y
  double w[NB][8];                               // sigma w
  float sigma = 1.0f, inv_sigma = 1.0f;
  bool degenerate = false;
  {
    const float* yrow = a.y + (int64_t)(p / a.y_rep) * a.ldy;
    float m = 0.0f;
#pragma unroll
    for (int q = 0; q < NB; ++q)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int t = MFMA_SPAN * q + tb + j;
        float yv;
        if (q == NB - 1) {
          const bool ok = t < a.N && !(j == 7 && g3);
          float yl = yrow[t < a.N ? t : a.N - 1];
          asm volatile("" : "+v"(yl));           // (the load stays unconditional)
          yv = ok ? yl : 0.0f;
        } else if (j == 7) {
          float yl = yrow[t];                    // (lane group 3: the first sample of block q+1, a valid address)
          asm volatile("" : "+v"(yl));
          yv = g3 ? 0.0f : yl;
        } else {
          yv = yrow[t];
        }
        ysn[q][j] = yv;
        m = fmaxf(m, fabsf(yv));
      }
    m = group_max(m);
    {
      const bool okm = m > 0.0f && m < 3.0e38f;
      int e = 0;
      (void)frexpf(okm ? m : 1.0f, &e);
      const float sg = ldexpf(1.0f, a.ybits - e) / y_scale, isg = ldexpf(1.0f, e - a.ybits) * y_scale;
      sigma = okm ? sg : 1.0f;
      inv_sigma = okm ? isg : 1.0f;
      degenerate = !okm && !a.cold;
    }
    const float ys = -sigma * y_scale;
    const double* wrow = a.w + (int64_t)p * a.ldw;
#pragma unroll
    for (int q = 0; q < NB; ++q)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        ysn[q][j] *= ys;
        w[q][j] = 0.0;
      }
    if (!a.cold) {                                // (the same for every lane: a scalar branch)
#pragma unroll
      for (int q = 0; q < NB; ++q)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int t = MFMA_SPAN * q + tb + j;
          if (q == NB - 1) {
            double wl = wrow[t < a.N ? t : a.N - 1] * (double)sigma;
            asm volatile("" : "+v"(wl));
            w[q][j] = (t < a.N && !(j == 7 && g3)) ? wl : 0.0;
          } else if (j == 7) {
            double wl = wrow[t] * (double)sigma;
            asm volatile("" : "+v"(wl));
            w[q][j] = g3 ? 0.0 : wl;
          } else {
            w[q][j] = wrow[t] * (double)sigma;
          }
        }
    }
  }
  const double th = lb * step * (double)sigma;
  const double nstep = -step * g_scale;
  const double nstep7 = g3 ? 0.0 : nstep;
  float guard = 0.0f, wlast = 0.0f;
  double unused0 = 0.0, unused1 = 0.0;           // (fista_update's sums of the stop rule: not in this variant)

  // tiles and -y in the accumulator half of the register file, as in fista_mfma_kernel
#pragma unroll
  for (int ps = 0; ps < 2; ++ps)
#pragma unroll
    for (int par = 0; par < 2; ++par)
#pragma unroll
      for (int r = 0; r < 2; ++r) asm volatile("" : "+a"(At[ps][par][r].hi), "+a"(At[ps][par][r].lo));
#pragma unroll
  for (int q = 0; q < NB; ++q)
#pragma unroll
    for (int j = 0; j < 8; ++j) asm volatile("" : "+a"(ysn[q][j]));

  u8 rth, rtl;                                   // the adjoint pass's B operand; the forward pass leaves the last block's fragment in it
  // slot -> (row half, split part): the sum row's half first
  // sl:  0      1      2      3      4      5
  //     r1 hh  r0 hh  r1 hl  r1 lh  r0 hl  r0 lh
  // ---- forward: r = T_c w - y, block by block (ascending); fragments of r go to LDS -------------
  auto forward = [&]() __attribute__((always_inline)) {
    u8 bh, bl;
    f4 acc[NB][2];
    float xf[NB][8];
    unsigned rh[NB][4], rl[NB][4];
    float remf = 0.0f;
    auto cvt_pair = [&](auto qc, auto pc) {       // slots 2p, 2p+1 of block q -> float32 (any time before the block's split)
      constexpr int q = decltype(qc)::value, pp = decltype(pc)::value;
      float x0, x1;                               // (asm: the conversion stays HERE, not behind the update)
      const double w0 = w[q][2 * pp], w1 = w[q][2 * pp + 1];
      asm volatile("v_cvt_f32_f64 %0, %1" : "=v"(x0) : "v"(w0));
      asm volatile("v_cvt_f32_f64 %0, %1" : "=v"(x1) : "v"(w1));
      xf[q][2 * pp] = x0;
      xf[q][2 * pp + 1] = x1;
    };
    auto split_block = [&](auto qc, auto pc) {    // -> the words of block q in the B operand (behind block q-1's last product)
      constexpr int q = decltype(qc)::value, pp = decltype(pc)::value;
      float x0 = xf[q][2 * pp], x1 = xf[q][2 * pp + 1];
      if constexpr (pp == 3 && q >= 1) {          // the sum slot: D_q = 2^-9 (w_0 + ... + w_{q-1}), finished by block q-1
        const float d = acc[q - 1][1][3] + remf;
        x1 = g3 ? d : x1;
      }
      unsigned h2, l2;
      if constexpr (PB_MFMA_REM && pp == 3 && q + 1 < NB) split_pair_rem(x0, x1, h2, l2, remf);
      else split_pair(x0, x1, h2, l2);
      bh[2 * pp + (q & 1)] = h2;
      bl[2 * pp + (q & 1)] = l2;
    };
    auto cinit = [&](auto qc, auto rc) {
      constexpr int q = decltype(qc)::value, r = decltype(rc)::value;
      acc[q][r] = f4{ysn[q][4 * r + 0], ysn[q][4 * r + 1], ysn[q][4 * r + 2], ysn[q][4 * r + 3]};
    };
    auto finish_pair = [&](auto qc, auto pc) {    // residual slots 2p, 2p+1 of block q -> fragment
      constexpr int q = decltype(qc)::value, pp = decltype(pc)::value;
      float x0 = acc[q][pp >> 1][(2 * pp) & 3], x1 = acc[q][pp >> 1][(2 * pp + 1) & 3];
      if constexpr (q == NB - 1) {                // padding behind sample N-1 and the sum slot (last block only)
        x0 = (MFMA_SPAN * q + tb + 2 * pp < a.N) ? x0 : 0.0f;
        x1 = (MFMA_SPAN * q + tb + 2 * pp + 1 < a.N && !(pp == 3 && g3)) ? x1 : 0.0f;
      }
      split_pair(x0, x1, rh[q][pp], rl[q][pp]);
      if constexpr (q == NB - 1) {                // the adjoint pass starts with this block: straight into its operand
        rth[2 * pp + (q & 1)] = rh[q][pp];
        rtl[2 * pp + (q & 1)] = rl[q][pp];
        rth[2 * pp + 1 - (q & 1)] = 0u;           // (no block behind it)
        rtl[2 * pp + 1 - (q & 1)] = 0u;
      }
      if constexpr (pp == 3) {
        lrf[(2 * q) * 64] = u4{rh[q][0], rh[q][1], rh[q][2], rh[q][3]};
        lrf[(2 * q + 1) * 64] = u4{rl[q][0], rl[q][1], rl[q][2], rl[q][3]};
      }
    };
    static_for<0, 4>([&](auto pc) {
      constexpr int pp = decltype(pc)::value;
      cvt_pair(std::integral_constant<int, 0>{}, pc);
      bh[2 * pp + 1] = 0u;                        // (no block before the first)
      bl[2 * pp + 1] = 0u;
    });
    static_for<0, 4>([&](auto pc) { split_block(std::integral_constant<int, 0>{}, pc); });
    cinit(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
    cinit(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
    static_for<0, NB>([&](auto qc) {
      constexpr int q = decltype(qc)::value;
      static_for<0, 6>([&](auto sc) {
        constexpr int sl = decltype(sc)::value;
        constexpr int r = (sl == 1 || sl >= 4) ? 0 : 1, part = sl < 2 ? 0 : (sl == 2 || sl == 4 ? 1 : 2);
        acc[q][r] = smfmac_part(At[0][q & 1][r], ai[0][q & 1][r], bh, bl, acc[q][r], part);
        // a slice of the neighbours' vector work: the residual of the block before, the next block's conversions and -y
        if constexpr (sl < 4) {
          if constexpr (q >= 1) finish_pair(std::integral_constant<int, q - 1>{}, sc);
          if constexpr (q + 1 < NB) cvt_pair(std::integral_constant<int, q + 1>{}, sc);
        } else {
          if constexpr (q + 1 < NB) cinit(std::integral_constant<int, q + 1>{}, std::integral_constant<int, sl - 4>{});
        }
      });
      // behind the block's last product: the next block's words (its sum slot waits for this block's sum row).  The
      // scheduler may not lift them over a product that reads the operand: it would copy the whole tuple to do so.
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (q + 1 < NB) static_for<0, 4>([&](auto pc) { split_block(std::integral_constant<int, q + 1>{}, pc); });
    });
    static_for<0, 4>([&](auto pc) { finish_pair(std::integral_constant<int, NB - 1>{}, pc); });
  };
  // ---- adjoint and update: g = T_c^T r, block by block (descending) ------------------------------
  auto backward = [&](const double beta) __attribute__((always_inline)) {
    const double nb1 = -(1.0 + beta);
    f4 acc[NB][2];
    unsigned fh3[NB], fl3[NB];                    // word 3 of a fetched fragment (slots 6, 7): rebuilt by `patch`
    float remb = 0.0f;
    const unsigned psel = g3 ? 0x07060100u : 0x03020100u;
    auto fetch = [&](auto qc) {                   // residual fragment of block q < NB-1: LDS -> its words of the operand
      constexpr int q = decltype(qc)::value;
      // (word by word, volatile, through LDS pointers: one 128-bit read lands in four adjacent registers and is moved
      // from there)
      typedef const volatile __attribute__((address_space(3))) unsigned lds_word;
      lds_word* ph3 = (lds_word*)reinterpret_cast<const unsigned*>(&lrf[(2 * q) * 64]);
      lds_word* pl3 = (lds_word*)reinterpret_cast<const unsigned*>(&lrf[(2 * q + 1) * 64]);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        rth[2 * c + (q & 1)] = ph3[c];
        rtl[2 * c + (q & 1)] = pl3[c];
      }
      fh3[q] = ph3[3];
      fl3[q] = pl3[3];
    };
    auto patch = [&](auto qc) {                   // the sum slot of block q: 2^-9 (r_{q+1} + ... + r_{NB-1}), finished by block q+1
      constexpr int q = decltype(qc)::value;
      const float d = acc[q + 1][1][3] + remb;
      const unsigned h2 = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(d, d));
      float l;
      asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(l) : "v"(h2), "v"(d));
      const unsigned l2 = pk_rne(l, l);
      if constexpr (PB_MFMA_REM && q >= 1) asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(remb) : "v"(l2), "v"(l));
      rth[6 + (q & 1)] = __builtin_amdgcn_perm(h2, fh3[q], psel);
      rtl[6 + (q & 1)] = __builtin_amdgcn_perm(l2, fl3[q], psel);
    };
    auto update = [&](auto qc, auto jc) {
      constexpr int q = decltype(qc)::value, j = decltype(jc)::value;
      (void)fista_update<false>(w[q][j], acc[q][j >> 2][j & 3], j == 7 ? nstep7 : nstep, th, nb1, unused0, unused1);
    };
    static_for<0, NB>([&](auto qq) {
      constexpr int q = NB - 1 - decltype(qq)::value;
      static_for<0, 6>([&](auto sc) {
        constexpr int sl = decltype(sc)::value;
        constexpr int r = (sl == 1 || sl >= 4) ? 0 : 1, part = sl < 2 ? 0 : (sl == 2 || sl == 4 ? 1 : 2);
        if constexpr (part == 0) acc[q][r] = smfmac_part(At[1][q & 1][r], ai[1][q & 1][r], rth, rtl, f4{0.f, 0.f, 0.f, 0.f}, 0);
        else acc[q][r] = smfmac_part(At[1][q & 1][r], ai[1][q & 1][r], rth, rtl, acc[q][r], part);
        // the update of the block behind (its accumulators are finished), four samples beside the products ...
        if constexpr (sl >= 1 && sl < 5) {
          if constexpr (q + 1 < NB) update(std::integral_constant<int, q + 1>{}, std::integral_constant<int, sl - 1>{});
        }
      });
      // ... behind the block's last product the next block's fragment is fetched over the words of block q+1, and the
      // other four samples cover the fetch and the wait for this block's sum row
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (q >= 1) fetch(std::integral_constant<int, q - 1>{});
      if constexpr (q + 1 < NB) static_for<4, 8>([&](auto jc) { update(std::integral_constant<int, q + 1>{}, jc); });
      if constexpr (q >= 1) patch(std::integral_constant<int, q - 1>{});
    });
    static_for<0, 8>([&](auto jc) { update(std::integral_constant<int, 0>{}, jc); });
  };
  auto range_check = [&]() {
    const float m = iterate_absmax<NB>(w);
    wlast = m;
    guard = __builtin_fmaxf(guard, __builtin_fmaxf(m, residual_guard<NB>(lrf)));
  };

  for (int it = 0; it < a.n_iter; ++it) {
    const double beta = a.betas[it];
    forward();
    backward(beta);
    if (PB_MFMA_CHECKS && (((it & 7) == 7) || (it == a.n_iter - 1) || (it == 0 && !a.cold))) range_check();
  }

  // ---- store (unscaled); a problem that came near the float16 range or is too sparse is handed back ----
  guard = group_max(guard);
  wlast = group_max(wlast);
  const bool bad = !(guard < 60000.0f) || degenerate || (a.rho_guard && wlast > 0.0f && (float)th > MFMA_RHO_MAX * wlast);
  if (live && !bad) {
    double* wrow = a.w + (int64_t)p * a.ldw;
#pragma unroll
    for (int q = 0; q < NB; ++q)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int t = MFMA_SPAN * q + tb + j;
        if (t < a.N && !(j == 7 && g3)) wrow[t] = w[q][j] * (double)inv_sigma;
      }
  }
  if (live && a.n_done && g == 0) a.n_done[p] = bad ? -1 : a.n_iter;
}

// the launch of fista_mfma_kernel's plain variant (launch_mfma_nt<NB, 2>), for K <= 32
template <int NB>
int launch_mfma_sparse(const FistaArgs& a, const double* taps, int K, hipStream_t st) {
  if (K < 1 || K > SPARSE_TILE_KMAX || a.N > MFMA_SPAN * NB || a.N <= MFMA_SPAN * (NB - 1)) return 1;
  const int64_t waves = (launch_count(a) + 15) / 16;
  const dim3 grid((unsigned)((waves + 3) / 4)), block(256);
  const size_t lds = (size_t)4 * NB * 2 * 64 * sizeof(u4) + 4 * 64 * sizeof(float);
  if (a.taps_pp) {                              // shared HRF and step in device memory
    const MfmaTaps none{};
    hipLaunchKernelGGL((fista_mfma_sparse_kernel<NB, true>), grid, block, lds, st, a, none);
    return 0;
  }
  const MfmaTaps tp = make_mfma_taps(taps, K);
  hipLaunchKernelGGL((fista_mfma_sparse_kernel<NB, false>), grid, block, lds, st, a, tp);
  return 0;
}

// what the dispatch calls for the one-wave matrix-pipe form: the plain solve (no cost trace, no stop rule; taps from the
// host or shared in device memory) with K <= 32 on the sparse tiles, every other call on fista_mfma_kernel's variants
template <int NB>
int launch_mfma_st(const FistaArgs& a, const double* taps, int K, bool with_j, hipStream_t st) {
  if (K <= SPARSE_TILE_KMAX && !with_j && a.stop_mode == PB_STOP_NONE) return launch_mfma_sparse<NB>(a, taps, K, st);
  return launch_mfma<NB>(a, taps, K, with_j, st);
}

}  // namespace pb
