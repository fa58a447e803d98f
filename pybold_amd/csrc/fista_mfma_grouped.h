// The one-wave matrix-pipe solve with ONE HRF PER PARCEL (pb_fista_solve_grouped): rows contiguous by parcel, taps
// [G][ldt] and steps [G] in device memory.  Mathematically G independent shared-HRF z-steps; here one launch whose waves
// each build their cumulative-tap table and operator tiles from their own parcel's row -- the GROUPED instantiations of
// fista_mfma_sparse_kernel (K <= 32: both near tiles in one 2:4-sparse product) and of fista_mfma_kernel (K = 33: two
// dense near tiles), exactly the two kernels the shared-HRF z-step runs on, so a parcel's rows come out as the shared
// form gives them for that parcel alone (the columns of a matrix product are independent).  129 .. 310 scans, plain
// solve: no stop rule, no cost trace.  The unit table (plan.h) says which rows a wave solves: FistaArgs::perm = the
// table, FistaArgs::n_dense = its length on the device, FistaArgs::grid_slots = the waves the host launches.
#pragma once
#include "fista_mfma_sparse.h"

namespace pb {

template <int NB>
int launch_mfma_grouped(const FistaArgs& a, int K, hipStream_t st) {
  if (K < 1 || K > 33 || a.N > MFMA_SPAN * NB || a.N <= MFMA_SPAN * (NB - 1)) return 1;
  if (!a.taps_pp || !a.step_vec || !a.perm || !a.n_dense || a.grid_slots < 1 || a.stop_mode != PB_STOP_NONE || a.y_rep != 1) return 1;
  const dim3 grid((unsigned)((a.grid_slots + 3) / 4)), block(256);
  const size_t lds = (size_t)4 * NB * 2 * 64 * sizeof(u4) + 4 * 64 * sizeof(float);      // residual fragments, taps
  const MfmaTaps none{};
  if (K <= SPARSE_TILE_KMAX) hipLaunchKernelGGL((fista_mfma_sparse_kernel<NB, true, true>), grid, block, lds, st, a, none);
  else hipLaunchKernelGGL((fista_mfma_kernel<NB, false, true, false, 2, false, true>), grid, block, lds, st, a, none);
  return 0;
}

}  // namespace pb
