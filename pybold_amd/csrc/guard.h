// The conditioning guard of the solves whose HRF lives in device memory (pb_fista_solve_pp_guarded,
// pb_fista_solve_grouped_guarded, pb_conditioning_marks): the host side of its device code.  The marks pass is path.h's
// marks_wave_kernel (launched by capi.hip); the kernels behind it -- the two lists built from the marks, the gather /
// scatter pair of the warm start -- live in guard_inst.hip alone, so that no other kernel object of the library changes.
//
// Workspace of a guarded call (int32 words, 8-byte aligned; pb_fista_guard_work_len):
//   [0, 8)                 header: {0, n64, 0, nv, 0, 0, 0, 0} -- words 0..1 are the range of the float64 list, 2..3 the
//                          range of the vector list (FistaArgs::range), so n64 = work[1] and nv = work[3]
//   marks   [P]            0 / 1 / 2 of every row
//   list64  [P]            rows with mark 2, ascending
//   listv   [P]            rows with mark 1, ascending (only when the call's route has a matrix-pipe form)
//   blocks  [2 nblk]       per-block counts, then their exclusive prefix
//   steps   [P] float64    one step per row for the float64 kernels of a shared-HRF call (they index step_vec per problem)
//   rows    [P][N] float64 the warm start of the listed rows: list64 from the front, listv from the back (not with
//                          PB_FLAG_COLD_START)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pb {

constexpr int GUARD_HEADER = 8;
constexpr int MARKS_KMAX = 64;             // = LMAX_KT
constexpr int MARKS_NMAX = 64 * 21;        // the longest strip of the marks pass

struct GuardLayout { int64_t marks, list64, listv, blocks, steps, rows, total; };
inline int64_t guard_blocks(int P) { return ((int64_t)P + 4095) / 4096; }
inline GuardLayout guard_layout(int P, int N, bool cold) {
  GuardLayout g;
  g.marks = GUARD_HEADER;
  g.list64 = g.marks + P;
  g.listv = g.list64 + P;
  g.blocks = g.listv + P;
  g.steps = (g.blocks + 2 * guard_blocks(P) + 1) & ~(int64_t)1;
  g.rows = g.steps + 2 * (int64_t)P;
  g.total = g.rows + (cold ? 0 : 2 * (int64_t)P * N);
  return g;
}

// the two lists and the header from the marks (`want_vec` = 0: the vector list stays empty)
void launch_mark_lists(int P, int want_vec, int32_t* work, const GuardLayout& g, hipStream_t st);
// steps[p] = step[0]
void launch_steps_fill(const double* step, double* steps, int P, hipStream_t st);
// the rows of w named by the two lists into `rows` (save = true) or back from it
void launch_rows_move(bool save, int P, int N, double* w, int64_t ldw, int32_t* work, const GuardLayout& g, hipStream_t st);

}  // namespace pb
