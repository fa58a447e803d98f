// The split matrix-pipe solves with ONE HRF PER PARCEL (pb_fista_solve_grouped with PB_FLAG_GROUPED_SPLIT): the GROUPED
// instantiations of fista_mfma2_kernel (311 .. 640 scans, two waves per 16 problems) and fista_mfma4_kernel (641 .. 1 280
// scans, four waves), with two near tiles (K <= 33) or three (34 .. 65 taps; the route serves up to 48, where the vector
// forms behind it end) -- the kernels the shared-HRF z-step runs on at these lengths (their TAPS_DEV instantiations), each
// WORKGROUP building its cumulative-tap table and operator tiles from its own parcel's row.  Plain solve: no stop rule, no
// cost trace.  The unit table is fista_mfma_grouped.h's (plan.h; units of 16 rows): FistaArgs::perm = the table,
// FistaArgs::n_dense = its length on the device, FistaArgs::grid_slots = the workgroups the host launches.
#pragma once
#include "fista_mfma4.h"

namespace pb {

// what launch_mfma_grouped refuses (fista_mfma_grouped.h)
inline bool grouped_split_args_ok(const FistaArgs& a, int K) {
  return K >= 1 && K <= 65 && a.taps_pp && a.step_vec && a.perm && a.n_dense && a.n_done && a.grid_slots >= 1 &&
         a.stop_mode == PB_STOP_NONE && a.y_rep == 1;
}

template <class Kernel>
void launch_grouped_split(Kernel kernel, const FistaArgs& a, unsigned threads, size_t lds, hipStream_t st) {
  // (more than 64 KB of dynamic LDS has to be asked for, per kernel and device: launch_mfma4 says so)
  if (lds > 65536) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kernel, dim3((unsigned)a.grid_slots), dim3(threads), lds, st, a, MfmaTaps{});
}

// 32 (NBA + NBB - 1) < N <= 32 (NBA + NBB), five blocks at least per wave (three near tiles need four)
template <int NBA, int NBB>
int launch_mfma2_grouped(const FistaArgs& a, int K, hipStream_t st) {
  constexpr int NB = NBA + NBB;
  static_assert(NBA > 3, "three near tiles: four blocks at least per wave");
  if (a.N > 32 * NB || a.N <= 32 * (NB - 1) || !grouped_split_args_ok(a, K)) return 1;
  const size_t lds = mfma2_lds_bytes(NBB);
  if (K > 33) launch_grouped_split(fista_mfma2_kernel<NBA, NBB, true, false, false, false, 3, true>, a, 128, lds, st);
  else launch_grouped_split(fista_mfma2_kernel<NBA, NBB, true, false, false, false, 2, true>, a, 128, lds, st);
  return 0;
}

// 128 (A - 1) < N <= 128 A
template <int A>
int launch_mfma4_grouped(const FistaArgs& a, int K, hipStream_t st) {
  if (a.N > 128 * A || a.N <= 128 * (A - 1) || !grouped_split_args_ok(a, K)) return 1;
  const size_t lds = mfma4_lds_bytes(A);
  if (K > 33) launch_grouped_split(fista_mfma4_kernel<A, true, false, false, false, 3, true>, a, 256, lds, st);
  else launch_grouped_split(fista_mfma4_kernel<A, true, false, false, false, 2, true>, a, 256, lds, st);
  return 0;
}

}  // namespace pb
