// Device side of the grouped calls' unit table (plan.h) and what pb_fista_solve_grouped needs around its solve.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "plan.h"

namespace pb {

constexpr int GROUPED_TABLE_THREADS = 256;

// first[G + 1] from the parcel offsets in device memory: ONE workgroup; thread t counts the units of its chunk of parcels
// (grouped_fill, the function the host build runs), a scan of the 256 counts numbers the chunks' first units, then
// every thread numbers the parcels of its chunk.  u_max: the units the table has room for (grouped_max_units: never
// reached by offsets the entry points accept; every number saturates there).
__global__ __launch_bounds__(GROUPED_TABLE_THREADS) void grouped_first_kernel(const int32_t* offsets, int G, int P, int per, int u_max,
                                                                              int32_t* first) {
  __shared__ int cnt[GROUPED_TABLE_THREADS];
  const int t = threadIdx.x;
  const int chunk = (G + GROUPED_TABLE_THREADS - 1) / GROUPED_TABLE_THREADS;
  const int g0 = t * chunk < G ? t * chunk : G, g1 = g0 + chunk < G ? g0 + chunk : G;
  cnt[t] = grouped_fill(offsets, g0, g1, P, per, 0, u_max, nullptr, nullptr);
  __syncthreads();
  int u0 = 0;
  for (int i = 0; i < t; ++i) u0 = cnt[i] < u_max - u0 ? u0 + cnt[i] : u_max;
  const int u1 = grouped_fill(offsets, g0, g1, P, per, u0, u_max, nullptr, first);
  if (t == GROUPED_TABLE_THREADS - 1) first[G] = u1;
}

// table[3 u ..], one thread per unit (a parcel of tens of thousands of rows has thousands of units: one thread filling
// them in turn took longer than the launch it prepares): the unit's parcel is the last one whose first unit is not
// behind it (binary search in first[], which skips empty parcels), its rows follow from its rank in the parcel --
// the entries grouped_fill writes on the host.
__global__ __launch_bounds__(GROUPED_TABLE_THREADS) void grouped_units_kernel(const int32_t* offsets, int G, int P, int per,
                                                                              const int32_t* first, int32_t* table) {
  const int u = blockIdx.x * GROUPED_TABLE_THREADS + threadIdx.x;
  if (u >= first[G]) return;
  int a = 0, b = G;                               // first[a] <= u < first[b]
  while (b - a > 1) {
    const int m = (a + b) >> 1;
    if (first[m] <= u) a = m; else b = m;
  }
  int lo, hi;
  grouped_range(offsets, a, P, lo, hi);
  const int r = lo + (u - first[a]) * per;
  table[GROUPED_WORDS * (int64_t)u] = r;
  table[GROUPED_WORDS * (int64_t)u + 1] = hi - r < per ? hi - r : per;
  table[GROUPED_WORDS * (int64_t)u + 2] = a;
}

// every row's copy of its parcel's HRF and step, [P][K] and [P]: what the per-problem vector forms read (the route of
// shapes without a matrix-pipe form, and the re-solve of what the matrix-pipe guards hand back).  One wave per unit.
__global__ __launch_bounds__(256) void grouped_expand_kernel(const int32_t* table, const int32_t* n_units, const double* taps,
                                                             int64_t ldt, int K, const double* step, double* taps_rows,
                                                             double* step_rows) {
  const int lane = threadIdx.x & 63;
  const int unit = (int)((blockIdx.x * 256 + threadIdx.x) >> 6);
  if (unit >= *n_units) return;
  const int32_t* ut = table + GROUPED_WORDS * (int64_t)unit;
  const int row0 = ut[0], rows = ut[1], parcel = ut[2];
  const double* src = taps + (int64_t)parcel * ldt;
  for (int i = lane; i < rows * K; i += 64) taps_rows[(int64_t)row0 * K + i] = src[i % K];
  if (lane < rows) step_rows[row0 + lane] = step[parcel];
}

}  // namespace pb
