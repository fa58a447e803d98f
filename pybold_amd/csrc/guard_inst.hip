// The device code of the conditioning guard for HRFs in device memory (guard.h) behind its marks pass (path.h:
// marks_wave_kernel, instantiated by capi.hip): the two lists, the step fill and the gather / scatter pair of the warm
// start.  One object of its own: every other kernel object of the library is built from the sources it was built from before.
#include "guard.h"

namespace pb {

namespace {

constexpr int PATH_THREADS = 256, PATH_PER_THREAD = 16, PATH_PER_BLOCK = PATH_THREADS * PATH_PER_THREAD;   // as path.h
static_assert(PATH_PER_BLOCK == 4096, "guard_blocks (guard.h) counts blocks of 4 096 rows");

// rows with mark 2 and (want_vec) mark 1 of every block of 4 096
__global__ __launch_bounds__(PATH_THREADS) void marks_count_kernel(const int32_t* marks, int P, int want_vec, int32_t* blocks) {
  __shared__ int part[2][PATH_THREADS / 64];
  const int p0 = blockIdx.x * PATH_PER_BLOCK + threadIdx.x * PATH_PER_THREAD;
  int c = 0, cv = 0;
  for (int i = 0; i < PATH_PER_THREAD; ++i) {
    if (p0 + i >= P) break;
    const int k = marks[p0 + i];
    c += k == 2;
    cv += (k == 1) & want_vec;
  }
  for (int o = 32; o > 0; o >>= 1) { c += __shfl_xor(c, o, 64); cv += __shfl_xor(cv, o, 64); }
  if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = c; part[1][threadIdx.x >> 6] = cv; }
  __syncthreads();
  if (threadIdx.x == 0) {
    blocks[blockIdx.x] = part[0][0] + part[0][1] + part[0][2] + part[0][3];
    blocks[gridDim.x + blockIdx.x] = part[1][0] + part[1][1] + part[1][2] + part[1][3];
  }
}

// exclusive prefix of the block counts (in place) and the header {0, n64, 0, nv, 0, 0, 0, 0} -- one workgroup
__global__ __launch_bounds__(PATH_THREADS) void marks_scan_kernel(int nblk, int32_t* blocks, int32_t* header) {
  __shared__ int buf[PATH_THREADS];
  __shared__ int carry;
  int total[2] = {0, 0};
  for (int which = 0; which < 2; ++which) {
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    int32_t* cnt = blocks + which * nblk;
    for (int b0 = 0; b0 < nblk; b0 += PATH_THREADS) {
      const int b = b0 + (int)threadIdx.x;
      const int v = b < nblk ? cnt[b] : 0;
      buf[threadIdx.x] = v;
      __syncthreads();
      for (int o = 1; o < PATH_THREADS; o <<= 1) {    // inclusive Hillis-Steele scan of 256 counts
        const int add = threadIdx.x >= (unsigned)o ? buf[threadIdx.x - o] : 0;
        __syncthreads();
        buf[threadIdx.x] += add;
        __syncthreads();
      }
      if (b < nblk) cnt[b] = carry + buf[threadIdx.x] - v;
      __syncthreads();
      if (threadIdx.x == PATH_THREADS - 1) carry += buf[PATH_THREADS - 1];
      __syncthreads();
    }
    total[which] = carry;
    __syncthreads();
  }
  if (threadIdx.x < GUARD_HEADER) header[threadIdx.x] = threadIdx.x == 1 ? total[0] : (threadIdx.x == 3 ? total[1] : 0);
}

// the lists: rows with mark 2 ascending in list64, rows with mark 1 ascending in listv
__global__ __launch_bounds__(PATH_THREADS) void marks_scatter_kernel(const int32_t* marks, int P, int want_vec, const int32_t* blocks,
                                                                     int32_t* list64, int32_t* listv) {
  __shared__ int buf[2][PATH_THREADS];
  const int p0 = blockIdx.x * PATH_PER_BLOCK + threadIdx.x * PATH_PER_THREAD;
  unsigned mask = 0, maskv = 0;
  int c = 0, cv = 0;
  for (int i = 0; i < PATH_PER_THREAD; ++i) {
    if (p0 + i >= P) break;
    const int k = marks[p0 + i];
    if (k == 2) { mask |= 1u << i; ++c; }
    if (k == 1 && want_vec) { maskv |= 1u << i; ++cv; }
  }
  buf[0][threadIdx.x] = c;
  buf[1][threadIdx.x] = cv;
  __syncthreads();
  for (int o = 1; o < PATH_THREADS; o <<= 1) {
    const int add = threadIdx.x >= (unsigned)o ? buf[0][threadIdx.x - o] : 0;
    const int addv = threadIdx.x >= (unsigned)o ? buf[1][threadIdx.x - o] : 0;
    __syncthreads();
    buf[0][threadIdx.x] += add;
    buf[1][threadIdx.x] += addv;
    __syncthreads();
  }
  int d = blocks[blockIdx.x] + buf[0][threadIdx.x] - c;                  // mark-2 rows before this thread's first one
  int e = blocks[gridDim.x + blockIdx.x] + buf[1][threadIdx.x] - cv;     // mark-1 rows before it
  for (int i = 0; i < PATH_PER_THREAD; ++i) {
    if (p0 + i >= P) break;
    if (mask & (1u << i)) list64[d++] = p0 + i;                          // (d < n64 <= P, e < nv <= P)
    else if (maskv & (1u << i)) listv[e++] = p0 + i;
  }
}

__global__ __launch_bounds__(256) void steps_fill_kernel(const double* step, double* steps, int P) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p < P) steps[p] = step[0];
}

// The warm start of the listed rows: position i of list64 lives in row i of `rows`, position j of listv in row P - 1 - j
// (n64 + nv <= P: the two never meet).  SAVE: rows <- w, else w <- rows.  The workgroups stride over the positions.
template <bool SAVE>
__global__ __launch_bounds__(256) void rows_move_kernel(const int32_t* header, const int32_t* list64, const int32_t* listv, int P, int N,
                                                        double* w, int64_t ldw, double* rows) {
  const int n64 = header[1], nv = header[3];
  for (int pos = blockIdx.x; pos < n64 + nv; pos += gridDim.x) {
    const int p = pos < n64 ? list64[pos] : listv[pos - n64];
    const int r = pos < n64 ? pos : P - 1 - (pos - n64);
    double* wr = w + (int64_t)p * ldw;
    double* sr = rows + (int64_t)r * N;
    for (int i = threadIdx.x; i < N; i += 256) {
      if (SAVE) sr[i] = wr[i];
      else wr[i] = sr[i];
    }
  }
}

}  // namespace

void launch_mark_lists(int P, int want_vec, int32_t* work, const GuardLayout& g, hipStream_t st) {
  const int nblk = (int)guard_blocks(P);
  hipLaunchKernelGGL(marks_count_kernel, dim3(nblk), dim3(PATH_THREADS), 0, st, work + g.marks, P, want_vec, work + g.blocks);
  hipLaunchKernelGGL(marks_scan_kernel, dim3(1), dim3(PATH_THREADS), 0, st, nblk, work + g.blocks, work);
  hipLaunchKernelGGL(marks_scatter_kernel, dim3(nblk), dim3(PATH_THREADS), 0, st, work + g.marks, P, want_vec, work + g.blocks,
                     work + g.list64, work + g.listv);
}

void launch_steps_fill(const double* step, double* steps, int P, hipStream_t st) {
  hipLaunchKernelGGL(steps_fill_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, step, steps, P);
}

void launch_rows_move(bool save, int P, int N, double* w, int64_t ldw, int32_t* work, const GuardLayout& g, hipStream_t st) {
  const dim3 grid((unsigned)(P < 2048 ? P : 2048)), block(256);
  double* rows = reinterpret_cast<double*>(work + g.rows);
  if (save)
    hipLaunchKernelGGL((rows_move_kernel<true>), grid, block, 0, st, work, work + g.list64, work + g.listv, P, N, w, ldw, rows);
  else
    hipLaunchKernelGGL((rows_move_kernel<false>), grid, block, 0, st, work, work + g.list64, work + g.listv, P, N, w, ldw, rows);
}

}  // namespace pb
