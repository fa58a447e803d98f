// C ABI of libpybold_hip.so (see include/pybold_hip.h for the contract and the
// reference interfaces each entry point replaces).
#include "../../include/pybold_hip.h"

#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>

#include "fista_fast.h"
#include "generic.h"
#include "launch_fast.h"
#include "fista_pair.h"
#include "fista_pair_ffa.h"
#include "fista_exact.h"
#include "fista_exact_split.h"
#include "fista_auto.h"
#include "fista_exact_pp.h"
#include "fista_exact_split_pp.h"
#include "blind.h"
#include "fista_mfma.h"
#include "fista_mfma_sparse.h"
#include "fista_mfma_row.h"
#include "fista_mfma_grouped.h"
#include "grouped.h"
#include "fista_mfma2.h"
#include "fista_mfma4.h"
#include "fista_mfma_split_grouped.h"
#include "path.h"
#include "guard.h"
#include "dispatch.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(PB_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
  g_err[0] = 0;
  return PB_OK;
}

constexpr int LDS_DOUBLES_MAX = 20000;  // 160 KB of LDS per workgroup
// the generic kernel's LDS in doubles: the row and two iterates, the taps, the reduction slots, the window rule's iterates
inline int64_t gen_lds_doubles(int N, int K, int stop_mode, int wind) {
  return 3 * (int64_t)N + K + 2 * pb::GEN_WAVES + (stop_mode == PB_STOP_WINDOW ? (int64_t)wind * N : 0);
}

// outer iterations per launch of a lambda search when the caller leaves the choice to the library: the form's budget of inner
// iterations per resident unit and launch over nb_sub_iter, fewer in proportion for a batch the machine does not hold at
// once, whose launch runs its units in rounds (the budgets and what they rest on: dispatch.h, kF64)
inline int auto_outer_chunk(int form, int V, int nb_sub_iter) {
  const F64FormDesc& d = kF64[form];
  const int64_t rounds = ((int64_t)V + d.auto_resident - 1) / d.auto_resident;
  const int64_t per = (int64_t)(nb_sub_iter > 0 ? nb_sub_iter : 1) * (rounds > 0 ? rounds : 1);
  const int64_t c = d.auto_launch_iters / per;
  return (int)(c < 1 ? 1 : c);
}

constexpr int MAD_DAUB_NMAX = 8192;
template <typename TY>
int mad_daub_impl(const TY* y_dev, int64_t ldy, int V, int N, double c, double* sigma_dev, void* stream, const char* name) {
  if (V < 0 || ldy < N) return fail(PB_ERR_INVALID, "%s: bad size", name);
  if (N < 5 || N > MAD_DAUB_NMAX) return fail(PB_ERR_INVALID, "%s: N=%d outside 5..%d scans", name, N, MAD_DAUB_NMAX);
  if (!(c > 0.0)) return fail(PB_ERR_INVALID, "%s: c must be positive", name);
  if (V == 0) return PB_OK;
  if (!y_dev || !sigma_dev) return fail(PB_ERR_INVALID, "%s: NULL pointer", name);
  int n2 = 1;
  while (n2 < (N + 5) / 2) n2 <<= 1;
  hipLaunchKernelGGL((pb::mad_daub_kernel<TY>), dim3(V), dim3(pb::GEN_THREADS), (size_t)n2 * sizeof(double), (hipStream_t)stream,
                     y_dev, ldy, N, c, n2, sigma_dev);
  return check_launch(name);
}
// ---- a side stream per device for remainders that fit BESIDE the main launch -----------
// When a plain solve has between one and two half rounds of pair waves (8 192 < P < 16 384
// problems on MI355X), a single launch leaves some SIMDs with two 8-problem waves and the
// others with one.  Measured (tools/conc_probe.py): half a round of pair waves (one per SIMD)
// on the caller's stream with the remainder on a second stream -- single-row waves (4
// problems) or one-problem waves -- co-schedules one wave of each per SIMD: 12 288 problems in
// 0.80 of a round instead of 0.92-1.0, 10 000 in 0.74.  The side stream forks from and joins
// back into the caller's stream with events (no host synchronisation); it is created on first
// use, one per device.  Not used while the caller's stream is being captured into a graph.  A
// remainder is never started beside a multi-round launch (measured slower: it unbalances the
// last round); after whole rounds the same group closes the plan (plan_pieces).
struct SideStream {
  hipStream_t stream = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  bool ok = false;
};
std::mutex g_side_mutex;

SideStream* side_stream_locked() {      // call with g_side_mutex held
  static std::map<int, SideStream> per_dev;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  SideStream& ss = per_dev[dev];
  if (!ss.ok && ss.stream == nullptr) {
    // Its own priority level: HIP multiplexes the streams of one priority onto a few hardware
    // queues, and a side stream that lands on the caller's queue runs BEHIND the caller's
    // kernel instead of beside it (seen after an application had created half a dozen streams)
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { least = greatest = 0; (void)hipGetLastError(); }
    if (hipStreamCreateWithPriority(&ss.stream, hipStreamNonBlocking, greatest) == hipSuccess &&
        hipEventCreateWithFlags(&ss.fork, hipEventDisableTiming) == hipSuccess &&
        hipEventCreateWithFlags(&ss.join, hipEventDisableTiming) == hipSuccess)
      ss.ok = true;
    else
      (void)hipGetLastError();
  }
  return ss.ok ? &ss : nullptr;
}

bool stream_is_capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) {
    (void)hipGetLastError();
    return true;                         // unknown: stay on one stream
  }
  return cs != hipStreamCaptureStatusNone;
}
// ---- workspace of a partitioned solve (int32 units) -----------------------------------------------------------
//   [0, P) the lists   [P] length of the front list   [P+1, P+1+nblk) block counts   ranges of the three lists'
//   candidate launches   lambda_max of every series (float64, when the caller has none)
//   ... then, for each of the three one-problem-per-wave candidates, three words s0 <= mid <= s1: its range cut at the end of
//   the dense class (path.h: path_scan_kernel) -- [s0, mid) for fista_mfma_row_kernel, [mid, s1) for the vector kernel
struct WorkLayout { int64_t ranges, split, lmax, total; };
WorkLayout work_layout(int P, int V) {
  const int64_t nblk = ((int64_t)P + pb::PATH_PER_BLOCK - 1) / pb::PATH_PER_BLOCK;
  WorkLayout w;
  w.ranges = ((int64_t)P + 2 + 2 * nblk + 8 + 1) & ~(int64_t)1;   // (list, n_front, front / ill counts per block, n_ill: path.h)
  w.split = w.ranges + 3 * 2 * pb::CAND_COUNT + 4;          // (3 x candidate ranges + the ill range)
  w.lmax = w.split + 3 * pb::WIDE_CANDS + 3;                // (even: 8-byte aligned when the buffer is)
  w.total = w.lmax + 2 * (int64_t)V + 8;
  return w;
}
// pb_fista_solve without a caller's workspace: one buffer per (device, stream), grown on demand, never freed
int32_t* own_workspace(void* stream, int64_t need, int64_t* len) {
  static std::mutex mu;
  static std::map<std::pair<int, void*>, std::pair<int32_t*, int64_t>> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  std::lock_guard<std::mutex> lock(mu);
  auto& e = cache[std::make_pair(dev, stream)];
  if (e.second < need) {
    int32_t* fresh = nullptr;
    const int64_t want = need + need / 4;
    if (hipMalloc((void**)&fresh, (size_t)want * sizeof(int32_t)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    // (the old buffer may still be read by work in flight on this stream: it is kept, not freed -- buffers grow by a
    // quarter at least, so what is retired over a process's life is a small multiple of the largest one)
    e.first = fresh;
    e.second = want;
  }
  *len = e.second;
  return e.first;
}

template <int KIND>
int launch_op(const double* x, int64_t ldx, double* out, int64_t ldo, int V, int n_src, int n_dst,
              const double* taps, int K, void* stream, const char* name) {
  // sizes first; an empty batch is a no-op whatever the pointers are (torch hands out
  // data_ptr() == 0 for zero-element tensors)
  if (V < 0 || n_src < 1 || n_dst < 1 || K < 0)
    return fail(PB_ERR_INVALID, "%s: bad size (V=%d n_src=%d n_dst=%d K=%d)", name, V, n_src, n_dst, K);
  if (ldx < n_src || ldo < n_dst) return fail(PB_ERR_INVALID, "%s: leading dimension too small", name);
  const int nmax = n_src > n_dst ? n_src : n_dst;
  if (2 * (int64_t)nmax + K + 8 > LDS_DOUBLES_MAX)
    return fail(PB_ERR_INVALID, "%s: row of %d with %d taps exceeds LDS", name, nmax, K);
  if (V == 0) return PB_OK;
  if (!x || !out || (K > 0 && !taps)) return fail(PB_ERR_INVALID, "%s: NULL pointer", name);
  const size_t lds = (size_t)(2 * nmax + K + 8) * sizeof(double);
  hipLaunchKernelGGL((pb::op_kernel<KIND>), dim3(V), dim3(pb::GEN_THREADS), lds, (hipStream_t)stream,
                     x, ldx, out, ldo, n_src, n_dst, taps, K);
  return check_launch(name);
}

template <bool CORR>
int launch_spectral(const double* x, int64_t ldx, double* out, int64_t ldo, int V, int N, const int32_t* map,
                    int L, int pad_left, const double* filt, int T, void* stream, const char* name) {
  if (V < 0 || N < 1 || L < N || T < 1 || T > L)
    return fail(PB_ERR_INVALID, "%s: bad size (V=%d N=%d L=%d T=%d; 1 <= N <= L and 1 <= T <= L required)", name,
                V, N, L, T);
  if (pad_left < 0 || pad_left > L - N)
    return fail(PB_ERR_INVALID, "%s: pad_left=%d outside [0, L - N] (N=%d L=%d)", name, pad_left, N, L);
  if (ldx < N || ldo < N) return fail(PB_ERR_INVALID, "%s: leading dimension too small", name);
  const int64_t nd = (int64_t)N + 2 * (int64_t)T - 1;        // window e[N + T - 1] and filter c[T]
  if (nd > LDS_DOUBLES_MAX)
    return fail(PB_ERR_INVALID, "%s: N=%d with T=%d filter taps exceeds LDS (N + 2 T - 1 = %lld > %d doubles)", name,
                N, T, (long long)nd, LDS_DOUBLES_MAX);
  if ((int64_t)V * pb::GEN_THREADS > (int64_t)UINT32_MAX) return fail(PB_ERR_INVALID, "%s: V=%d rows per launch", name, V);
  if (V == 0) return PB_OK;
  if (!x || !out || !map || !filt) return fail(PB_ERR_INVALID, "%s: NULL pointer", name);
  hipLaunchKernelGGL((pb::spectral_kernel<CORR>), dim3(V), dim3(pb::GEN_THREADS), (size_t)nd * sizeof(double),
                     (hipStream_t)stream, x, ldx, out, ldo, N, map, L, pad_left, filt, T);
  return check_launch(name);
}

}  // namespace

namespace {
template <typename TY>
int stats_impl(const double* w_dev, int64_t ldw, const TY* y_dev, int64_t ldy, int y_rep, int P,
               int N, const double* taps_dev, int K, double* r2_dev, double* l1_dev, void* stream,
               const char* name) {
  if (P < 0 || N < 1 || K < 1 || y_rep < 1 || ldw < N || ldy < N)
    return fail(PB_ERR_INVALID, "%s: bad size", name);
  if (2 * (int64_t)N + K + 8 > LDS_DOUBLES_MAX)
    return fail(PB_ERR_INVALID, "%s: N=%d K=%d exceeds LDS", name, N, K);
  if (P == 0) return PB_OK;
  if (!w_dev || !y_dev || !taps_dev || !r2_dev || !l1_dev)
    return fail(PB_ERR_INVALID, "%s: NULL pointer", name);
  const size_t lds = (size_t)(2 * N + K + 8) * sizeof(double);
  hipLaunchKernelGGL((pb::stats_kernel<TY>), dim3(P), dim3(pb::GEN_THREADS), lds,
                     (hipStream_t)stream, w_dev, ldw, y_dev, ldy, y_rep, N, taps_dev, K, r2_dev,
                     l1_dev);
  return check_launch(name);
}

template <typename TY>
int hrf_cost_impl(const double* z_dev, int64_t ldz, const TY* y_dev, int64_t ldy, int V, int N,
                  const double* taps_dev, int K, int n_hrf, double* cost_dev, int per_voxel,
                  void* stream, const char* name) {
  if (V < 0 || N < 1 || K < 1 || n_hrf < 1 || ldz < N || ldy < N)
    return fail(PB_ERR_INVALID, "%s: bad size", name);
  if (n_hrf > 65535) return fail(PB_ERR_INVALID, "%s: more than 65535 candidate HRFs", name);
  if ((int64_t)N + K + 8 > LDS_DOUBLES_MAX) return fail(PB_ERR_INVALID, "%s: exceeds LDS", name);
  if (V == 0) return PB_OK;
  if (!z_dev || !y_dev || !taps_dev || !cost_dev) return fail(PB_ERR_INVALID, "%s: NULL pointer", name);
  const size_t lds = (size_t)(N + K + 8) * sizeof(double);
  hipLaunchKernelGGL((pb::hrf_cost_kernel<TY>), dim3(V, n_hrf), dim3(pb::GEN_THREADS), lds,
                     (hipStream_t)stream, z_dev, ldz, y_dev, ldy, V, N, taps_dev, K, cost_dev,
                     per_voxel);
  return check_launch(name);
}
}  // namespace

namespace {
template <typename TY>
int lambda_max_impl(const TY* y_dev, int64_t ldy, int V, int N, const double* taps_dev, int K,
                    double* out_dev, void* stream, const char* name) {
  if (V < 0 || N < 1 || K < 1 || ldy < N) return fail(PB_ERR_INVALID, "%s: bad size", name);
  if (2 * (int64_t)N + K + 8 > LDS_DOUBLES_MAX)
    return fail(PB_ERR_INVALID, "%s: N=%d K=%d exceeds LDS", name, N, K);
  if (V == 0) return PB_OK;
  if (!y_dev || !taps_dev || !out_dev) return fail(PB_ERR_INVALID, "%s: NULL pointer", name);
  const size_t lds = (size_t)(2 * N + K + 8) * sizeof(double);
  hipLaunchKernelGGL((pb::lambda_max_kernel<TY>), dim3(V), dim3(pb::GEN_THREADS), lds,
                     (hipStream_t)stream, y_dev, ldy, N, taps_dev, K, out_dev);
  return check_launch(name);
}

constexpr int NE_MAX_BLOCKS = 2048;
constexpr int NE_WAVE_BLOCKS = 1024;           // one-voxel-per-wave form: one resident pass (4 workgroups per CU)

// the one-voxel-per-wave form serves K <= 32 (tail entries in registers) while four staging areas fit
inline bool ne_wave_form(int N, int K) {
#ifdef PB_DEVELOPMENT                            // A/B aid of development builds only: the release library reads no environment
  if (getenv("PB_NE_BLOCK_FORM")) return false;
#endif
  return K <= 32 && (int64_t)pb::ne_wave_lds_doubles(N, K) <= LDS_DOUBLES_MAX;
}
inline int ne_wave_blocks(int V, int cap) {
  int b = (V + pb::GEN_WAVES - 1) / pb::GEN_WAVES;
  if (b > NE_WAVE_BLOCKS) b = NE_WAVE_BLOCKS;
  return b < cap ? b : cap;
}

template <typename TY>
int normal_eq_impl(const double* z_dev, int64_t ldz, const TY* y_dev, int64_t ldy, int V, int N,
                   int K, int per_voxel, double* work_dev, int64_t work_len, double* out_dev,
                   void* stream, const char* name) {
  if (V < 0 || N < 1 || K < 1 || K > 127 || ldz < N || ldy < N)
    return fail(PB_ERR_INVALID, "%s: bad size (V=%d N=%d K=%d)", name, V, N, K);
  const int ne = pb::ne_len(K);
  int sub_log2 = 0;                            // lanes per role: 4 for K <= 31, 2 for K <= 63
  while ((2 * K + 1) << (sub_log2 + 1) <= pb::NE_THREADS && sub_log2 < 2) ++sub_log2;
  const int64_t nd = per_voxel ? 2 * (int64_t)N : (int64_t)pb::ne_sum_lds_doubles(N, K);
  if (nd > LDS_DOUBLES_MAX) return fail(PB_ERR_INVALID, "%s: N=%d K=%d exceeds LDS", name, N, K);
  const size_t lds = (size_t)nd * sizeof(double);
  if (per_voxel) {
    if (V == 0) return PB_OK;
    if (!z_dev || !y_dev || !out_dev) return fail(PB_ERR_INVALID, "%s: NULL pointer", name);
    hipLaunchKernelGGL((pb::normal_eq_kernel<TY>), dim3(V < 65536 ? V : 65536),
                       dim3(pb::NE_THREADS), lds, (hipStream_t)stream, z_dev, ldz, y_dev, ldy, V, N, K,
                       sub_log2, out_dev);
    return check_launch(name);
  }
  // shared mode: block partials in work_dev, then a fixed-order sum (an empty shard yields
  // zeros, so that the rank still contributes to the all-reduce)
  if (!out_dev) return fail(PB_ERR_INVALID, "%s: NULL output", name);
  int blocks = V < NE_MAX_BLOCKS ? V : NE_MAX_BLOCKS;
  if (work_len / ne < blocks) blocks = (int)(work_len / ne);
  if (V > 0) {
    if (blocks < 1 || !work_dev)
      return fail(PB_ERR_INVALID, "%s: work buffer must hold at least %d doubles", name, ne);
    if (!z_dev || !y_dev) return fail(PB_ERR_INVALID, "%s: NULL pointer", name);
    if (ne_wave_form(N, K)) {                  // one voxel per wave (blind.h)
      blocks = ne_wave_blocks(V, blocks);
      hipLaunchKernelGGL((pb::normal_eq_wave_kernel<TY, false>), dim3(blocks), dim3(pb::NE_THREADS),
                         (size_t)pb::ne_wave_lds_doubles(N, K) * sizeof(double), (hipStream_t)stream, z_dev,
                         ldz, y_dev, ldy, V, N, K, work_dev);
    } else {
      hipLaunchKernelGGL((pb::normal_eq_sum_kernel<TY>), dim3(blocks), dim3(pb::NE_THREADS),
                         (size_t)pb::ne_sum_lds_doubles(N, K) * sizeof(double), (hipStream_t)stream, z_dev,
                         ldz, y_dev, ldy, V, N, K, work_dev);
    }
  } else {
    blocks = 0;
  }
  hipLaunchKernelGGL(pb::normal_eq_reduce_kernel, dim3(ne), dim3(pb::NE_THREADS), 0,
                     (hipStream_t)stream, work_dev, blocks, ne, out_dev);
  return check_launch(name);
}
}  // namespace


namespace {
// ---- running a route --------------------------------------------------------------------------------------------------
// launch_form(form, args, stream, exact_rule) -> 0 / 1 (rejected): the kernel launcher the route holds for a form of the
// plan (plan.h); exact_rule = the window rule in full, not as a certificate (re-solves of handed-back problems).  One
// mapping per call kind, built once per call from its Route; the executors below take either.
struct HostTapsForms {            // pb_fista_solve, _ex, _path: the taps on the host
  const Route& r;
  const char* name;               // the entry point, for error texts
  const double* taps;
  int K, stop_mode;
  bool wj, direct_fir;
  int operator()(int form, const pb::FistaArgs& b, hipStream_t st, bool exact_rule) const {
    const bool cert = r.cert && !exact_rule;
    switch (form) {
      case FORM_MFMA: return r.mfma ? r.mfma(b, taps, K, wj, st) : 1;
      case FORM_MFMA2: return r.split ? r.split(b, taps, K, wj, st) : 1;      // (over four waves beyond 640 scans)
      case FORM_PAIR:
        if (r.path == PATH_PART_LONG || r.path == PATH_SPLIT_PAIR) return r.se->fn_pair_split(b, taps, K, wj, cert, st);
        if (cert) return r.fe->fn_pair_cert(b, taps, K, st);
        return ((r.fe->fn_pair_ffa && !direct_fir) ? r.fe->fn_pair_ffa : r.fe->fn_pair)(b, taps, K, wj, st);
      case FORM_WIDE: return r.we ? r.we->fn(b, taps, K, wj, stop_mode, st) : 1;
      default: return r.fe->fn(b, taps, K, wj, stop_mode, st);
    }
  }
};
struct DeviceTapsForms {          // pb_fista_solve_pp: taps and steps in device memory (FistaArgs::taps_pp, step_vec)
  const Route& r;
  const char* name;
  int K, stop_mode;
  int operator()(int form, const pb::FistaArgs& b, hipStream_t st, bool) const {
    switch (form) {
      case FORM_MFMA: return r.mfma ? r.mfma(b, nullptr, K, false, st) : 1;
      case FORM_MFMA2: return r.split ? r.split(b, nullptr, K, false, st) : 1;
      case FORM_PAIR: return r.fe->fn_pair_dev(b, st);
      case FORM_WIDE: return r.we ? r.we->fn_pp(b, stop_mode, st) : 1;
      default: return r.fe->fn_pp(b, stop_mode, st);
    }
  }
};

template <class LF>
int launch(const LF& lf, int form, const pb::FistaArgs& b, hipStream_t st, bool exact_rule = false) {
  static const char* const kernel[] = {"fista_generic_kernel", "fista_fast_kernel", "fista_pair_ffa_kernel", "fista_fast_kernel(wide)",
                                       "fista_mfma_kernel", "fista_mfma2_kernel / fista_mfma4_kernel"};
  if (lf(form, b, st, exact_rule) != 0) return fail(PB_ERR_INVALID, "%s: the kernel of form %d rejected its launch", lf.name, form);
  return check_launch(kernel[form]);
}

// The device's side stream in the hands of one call: taken under the lock, forked from the caller's stream once, joined back
// into it if it was forked
struct Side {
  std::unique_lock<std::mutex> lock{g_side_mutex, std::defer_lock};
  SideStream* ss = nullptr;
  bool forked = false;
  void take() {
    lock.lock();
    ss = side_stream_locked();
  }
  int fork(hipStream_t user, const char* name) {
    if (forked) return PB_OK;
    if (hipEventRecord(ss->fork, user) != hipSuccess || hipStreamWaitEvent(ss->stream, ss->fork, 0) != hipSuccess)
      return fail(PB_ERR_HIP, "%s: fork to the side stream failed", name);
    forked = true;
    return PB_OK;
  }
  int join(hipStream_t user, const char* name) {
    if (!forked) return PB_OK;
    forked = false;
    if (hipEventRecord(ss->join, ss->stream) != hipSuccess || hipStreamWaitEvent(user, ss->join, 0) != hipSuccess)
      return fail(PB_ERR_HIP, "%s: join of the side stream failed", name);
    return PB_OK;
  }
};

// Whole passes [0, base) on a matrix-pipe form (`main_form`), the remainder [base, P) on a vector form (`rest_form`), then
// `rest_form` again over [0, base) for the problems the main form's guards handed back (only_flagged: n_done = -1)
template <class LF>
int run_passes(const pb::FistaArgs& a, int base, int main_form, int rest_form, bool resolve, const LF& lf, hipStream_t st) {
  pb::FistaArgs b = a;
  if (base > 0) {
    b.P = base;
    const int rc = launch(lf, main_form, b, st);
    if (rc != PB_OK) return rc;
  }
  if (base < a.P) {
    b = a;
    b.p0 = base;
    const int rc = launch(lf, rest_form, b, st);
    if (rc != PB_OK) return rc;
  }
  if (base > 0 && resolve) {
    b = a;
    b.P = base;
    b.only_flagged = 1;
    return launch(lf, rest_form, b, st, true);
  }
  return PB_OK;
}

// The host-side plan of a single-row entry's shape: whole rounds on the densest form, the remainder on the cheapest (the pair
// form has no stop rules; the one-problem-per-wave form has them all); a remainder that fits beside half a round of pair
// waves runs on the side stream.  Then the flagged problems of the pieces that may leave n_done = -1: the exact rule on the
// single-row form, on the caller's stream (after the join)
template <class LF>
int run_pieces(const Route& r, const pb::FistaArgs& a, const LF& lf, hipStream_t user, unsigned flags) {
  Piece pc[pb::MAX_PIECES];
  const bool one_stream = r.one_stream || r.one_form || (flags & PB_FLAG_ONE_STREAM) != 0 || stream_is_capturing(user);
  const int npc = route_pieces(r, a.P, (flags & PB_FLAG_ONE_LAUNCH) != 0, one_stream, pc);
  bool any_side = false;
  int q0 = a.P, q1 = 0;                          // range of the pieces that may leave n_done = -1 (contiguous)
  for (int i = 0; i < npc; ++i) {
    any_side |= pc[i].side;
    if ((pc[i].form == FORM_PAIR && r.cert) || pc[i].form == FORM_MFMA || pc[i].form == FORM_MFMA2) {
      q0 = pc[i].p0 < q0 ? pc[i].p0 : q0;
      q1 = pc[i].p1 > q1 ? pc[i].p1 : q1;
    }
  }
  Side side;
  if (any_side) side.take();                     // (no side stream: the same pieces, one after the other)
  pb::FistaArgs b = a;
  int rc = PB_OK;
  for (int i = 0; i < npc && rc == PB_OK; ++i) {
    if (pc[i].group && side.ss) rc = side.fork(user, lf.name);   // whole rounds are in the queue: the group starts here
    if (rc != PB_OK) break;
    b.p0 = pc[i].p0;
    b.P = pc[i].p1;
    rc = launch(lf, pc[i].form, b, (pc[i].side && side.ss) ? side.ss->stream : user);
  }
  // join even after an error so that the caller's stream never runs ahead of the side stream
  const int rj = side.join(user, lf.name);
  if (rj != PB_OK) return rj;
  if (rc != PB_OK || q1 <= q0 || (flags & PB_FLAG_CERT_NO_RESOLVE)) return rc;
  b.p0 = q0;
  b.P = q1;
  b.only_flagged = 1;
  return launch(lf, FORM_FAST1, b, user, true);
}

// a route that solves the problems where they lie (no partition): every call of pb_fista_solve_pp, and of pb_fista_solve below
// PART_MIN_P problems, without a workspace or under a pin
template <class LF>
int run_in_place(const Route& r, const pb::FistaArgs& a, const LF& lf, hipStream_t user, unsigned flags) {
  const bool resolve = !(flags & PB_FLAG_CERT_NO_RESOLVE);
  switch (r.path) {
    case PATH_SPLIT_LONG: return run_passes(a, r.base, FORM_MFMA2, r.backup_wide ? FORM_WIDE : FORM_FAST1, resolve, lf, user);
    case PATH_MFMA_WIDE: return run_passes(a, r.base, FORM_MFMA, FORM_WIDE, resolve, lf, user);
    // (every series on the split pair form, the certificate's re-solve one problem per wave)
    case PATH_SPLIT_PAIR: return run_passes(a, a.P, FORM_PAIR, FORM_WIDE, r.cert && resolve, lf, user);
    case PATH_PIECES: return run_pieces(r, a, lf, user, flags);
    case PATH_WIDE: return launch(lf, FORM_WIDE, a, user);
    default: return fail(PB_ERR_INVALID, "%s: this route is not solved in place", lf.name);
  }
}

// ---- the partition BEFORE solving (dense class -> matrix pipe, sparse class -> float32 vector forms) and a compacted
// re-solve of what a guard or certificate hands back; list lengths and launch plans live on the device (path.h, plan.h).
// Without it a batch whose lambda lies near lambda_max was solved twice -- matrix pipe, then one handed-back problem per
// wave (profiles/r4_path_partition.txt: 2.05 against 3.20e9).
struct PartitionSpecs { pb::PlanSpec dense, sparse, flagged; };
PartitionSpecs partition_specs(const Route& r, int N, bool one_stream) {
  const double slots = wave_slots();
  const int pair = r.has_pair ? 1 : 0, wide = r.has_wide ? 1 : 0, os = one_stream ? 1 : 0;
  if (r.path == PATH_PART_SHORT)
    return {{1, pair, wide, 0, os, r.has_mfma2 ? 1 : 0, r.beside_chunks, slots}, {2, pair, wide, 0, os, 0, 0, slots}, {2, 0, wide, 0, 1, 0, 0, slots}};
  PartitionSpecs s{{3, 0, 0, 0, 1, 1, 0, slots}, {4, pair, 0, 0, 1, 0, 0, slots}, {4, 0, 0, 0, 1, 0, 0, slots}};
  if (N > 640) {                                 // 641 .. 1 280 scans: the form split over four waves (fista_mfma4.h)
    s.dense.pass_mult = 2;
    s.dense.rem_num16 = MFMA4_MIN_R_NUM;
  }
  s.dense.backup_form = s.sparse.backup_form = s.flagged.backup_form = r.backup_wide ? FORM_WIDE : FORM_FAST1;
  s.sparse.min_pair = SPLIT_MIN_P;
  return s;
}
// which candidate launches of a list exist (list 0: the call's one list -- matrix-pipe forms for its dense head, vector forms
// for the rest --, 1 / 2: the measurement aids "matrix-pipe candidates only" / "vector candidates only", 3: handed-back problems)
bool list_has_form(const Route& r, int form, int list) {
  const bool lng = r.path == PATH_PART_LONG;
  if (form == FORM_MFMA) return list <= 1 && r.mfma != nullptr;
  if (form == FORM_MFMA2) return list <= 1 && (lng || r.has_mfma2);
  if (list == 1) return false;
  if (form == FORM_PAIR) return list != 3 && r.has_pair;
  if (form == FORM_WIDE) return lng ? r.backup_wide : r.has_wide;
  return !lng || !r.backup_wide;
}
// grid bound of a candidate in slots
int cand_bound(const Route& r, int c, int P) {
  if (r.path == PATH_PART_SHORT) return pb::cand_max_slots(c, P, wave_slots());
  return (c == pb::CAND_MFMA2 || c == pb::CAND_PAIR0 || c == pb::CAND_FAST0 || c == pb::CAND_WIDE) ? P : 0;
}

// a whole list: its candidates in their static order, the side-stream ones forked after the whole rounds
template <class LF>
int solve_list(const Route& r, const pb::FistaArgs& a, const LF& lf, hipStream_t user, Side& side, const int32_t* work_dev,
               const int32_t* ranges, int list, bool exact_rule, const int32_t* split = nullptr, const double* taps_host = nullptr) {
  pb::FistaArgs b = a;
  b.perm = work_dev;
  b.n_dense = work_dev + a.P;
  b.perm_side = list == 3 ? 3 : 1;
  int rc = PB_OK;
  for (int c = 0; c < pb::CAND_COUNT && rc == PB_OK; ++c) {
    const int form = pb::cand_form(c);
    if (!list_has_form(r, form, list) || (pb::cand_side(c) && !side.ss)) continue;
    // (a plan on one stream has no groups, and a second piece of a form continues the first: plan_to_candidates merges them)
    if ((c == pb::CAND_PAIR1 || c == pb::CAND_FAST1) && !side.ss) continue;
    b.grid_slots = cand_bound(r, c, a.P);
    if (b.grid_slots <= 0) continue;
    if (c >= pb::CAND_FIRST_AFTER_FORK && side.ss) rc = side.fork(user, lf.name);
    if (rc != PB_OK) break;
    b.range = ranges + 2 * c;
    const hipStream_t st = (pb::cand_side(c) && side.ss) ? side.ss->stream : user;
    if (split && form == FORM_WIDE) {
      // the dense rows of this range, [s0, mid), one series per wave on the matrix pipe (fista_mfma_row.h); the vector
      // kernel right behind it, launched as ever, with what is left of the range
      const int32_t* cut = split + 3 * pb::wide_cand_index(c);
      b.range = cut;
      rc = pb::launch_mfma_row(b, taps_host, a.K, false, st) != 0
               ? fail(PB_ERR_INVALID, "%s: fista_mfma_row_kernel rejected its launch", lf.name)
               : check_launch("fista_mfma_row_kernel");
      if (rc != PB_OK) break;                      // (the join below still runs)
      b.range = cut + 1;
    }
    rc = launch(lf, form, b, st, exact_rule);
  }
  const int rj = side.join(user, lf.name);
  return rj != PB_OK ? rj : rc;
}

// lambda_max of every series, with max|y| and the marks of the ill-conditioned ones -- float32, ~55 us per 100 k series
// (gamma_f64, gamma_vec: the coherence bounds below which a series is marked for the float64 kernel / kept off the matrix pipe; 0: none)
void launch_lmax_pass(const pb::FistaArgs& a, int V_series, const double* taps_host, double* lm, double gamma_f64, double gamma_vec,
                      hipStream_t st) {
  const int N = a.N, K = a.K;
  pb::LmaxTaps lt;
  double run = 0.0, csum = 0.0;                   // sum|c| over the N lags of the operator's step response c = cumsum(h)
  for (int k = 0; k < pb::LMAX_KT; ++k) lt.h[k] = k < K ? (float)taps_host[k] : 0.0f;
  for (int t = 0; t < N; ++t) { if (t < K) run += taps_host[t]; csum += std::fabs(run); }
  const double unit = csum / std::sqrt((double)N);
  const float f64_bound = gamma_f64 > 0.0 ? (float)(gamma_f64 * unit) : 0.0f, vec_bound = gamma_vec > 0.0 ? (float)(gamma_vec * unit) : 0.0f;
  const dim3 grid((unsigned)((V_series + 3) / 4)), block(256);
  if (N <= 320) hipLaunchKernelGGL((pb::lmax_wave_kernel<5>), grid, block, 4 * (64 * 5 + pb::LMAX_KT) * sizeof(float), st, a.y, a.ldy, V_series, N, lt, K, lm, f64_bound, vec_bound);
  else if (N <= 640) hipLaunchKernelGGL((pb::lmax_wave_kernel<10>), grid, block, 4 * (64 * 10 + pb::LMAX_KT) * sizeof(float), st, a.y, a.ldy, V_series, N, lt, K, lm, f64_bound, vec_bound);
  else hipLaunchKernelGGL((pb::lmax_wave_kernel<21>), grid, block, 4 * (64 * 21 + pb::LMAX_KT) * sizeof(float), st, a.y, a.ldy, V_series, N, lt, K, lm, f64_bound, vec_bound);   // (odd strips: conflict-free)
}

// count, scan (which also plans the lists: plan_kernel's work on thread 0) and scatter of one class predicate
int launch_partition(const pb::ClassPred& cp, int P, int32_t* work_dev, const pb::PlanSpec& front, const pb::PlanSpec& back,
                     int32_t* rg_front, int32_t* rg_back, int32_t* rg_ill, const char* what, hipStream_t st, int32_t* rg_split = nullptr) {
  const int nblk = (P + pb::PATH_PER_BLOCK - 1) / pb::PATH_PER_BLOCK;
  hipLaunchKernelGGL(pb::path_count_kernel, dim3(nblk), dim3(pb::PATH_THREADS), 0, st, cp, P, work_dev);
  hipLaunchKernelGGL(pb::path_scan_kernel, dim3(1), dim3(pb::PATH_THREADS), 0, st, P, nblk, work_dev, front, back, rg_front, rg_back, rg_ill, rg_split);
  hipLaunchKernelGGL(pb::path_scatter_kernel, dim3(nblk), dim3(pb::PATH_THREADS), 0, st, cp, P, work_dev);
  return check_launch(what);
}

// the any-size LDS kernel (generic.h), one workgroup per problem (fewer: they stride over a device-side list)
void launch_generic(const pb::FistaArgs& a, const double* taps_dev, int K, int wind, bool with_j, bool f64, int grid, hipStream_t st) {
  void (*const kernel)(pb::FistaArgs, const double*, int, int) =
      !f64 ? (with_j ? pb::fista_generic_kernel<true> : pb::fista_generic_kernel<false>)
           : (with_j ? pb::fista_generic_kernel<true, true> : pb::fista_generic_kernel<false, true>);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(pb::GEN_THREADS), (size_t)gen_lds_doubles(a.N, K, a.stop_mode, wind) * sizeof(double), st,
                     a, taps_dev, K, wind);
}

template <class LF>
int run_partition(const Route& r, const pb::FistaArgs& a, const LF& lf, hipStream_t user, const double* taps_host,
                  const double* taps_dev, unsigned flags, double dense_ratio, int32_t* work_dev) {
  const int P = a.P, N = a.N, K = a.K, V_series = (P + a.y_rep - 1) / a.y_rep;
  const bool one_stream = r.path == PATH_PART_LONG || (flags & PB_FLAG_ONE_STREAM) != 0 || stream_is_capturing(user);
  const PartitionSpecs sp = partition_specs(r, N, one_stream);
  const WorkLayout wl = work_layout(P, V_series);
  // The ill-conditioned class (marked by the lambda_max pass, the tail of the list array) goes to a float64 kernel, any stop
  // rule: the register-resident one, one or four waves per series, where the shape has an entry (its window rule is
  // wind = 6; 1.0e9 voxel-iterations/s against 0.17e9), else the LDS one, which needs the taps in device memory and the row
  // in LDS; with neither, or without the guard, no series is marked
  const ExactEntry* ill_exact = pick_f64_default(N, K, a.stop_mode, a.wind, true);
  const bool ill_generic = !ill_exact && taps_dev && gen_lds_doubles(N, K, a.stop_mode, a.wind) <= LDS_DOUBLES_MAX;
  const bool guard = !(flags & PB_FLAG_NO_ILL_GUARD);
  // (the caller's lmax_dev is not needed: the pass also sees max|y| and marks the ill-conditioned series, which the caller's
  // numbers do not tell)
  double* lmax = reinterpret_cast<double*>(work_dev + wl.lmax);
  launch_lmax_pass(a, V_series, taps_host, lmax, (guard && (ill_exact || ill_generic)) ? PART_GAMMA_F64 : 0.0,
                   guard ? part_gamma_matrix_pipe(N, K) : 0.0, user);
  int32_t* rg_dense = work_dev + wl.ranges;
  int32_t* rg_sparse = rg_dense + 2 * pb::CAND_COUNT;
  int32_t* rg_flag = rg_sparse + 2 * pb::CAND_COUNT;
  int32_t* rg_ill = rg_flag + 2 * pb::CAND_COUNT;
  const double ratio = (r.path == PATH_PART_SHORT && !r.mfma) ? 0.0                    // (no matrix-pipe form: no dense class)
                       : dense_ratio > 0.0 ? dense_ratio
                       : N > 640 ? PB_PATH_DENSE_RATIO_LONGER : (N > MFMA1_NMAX ? PB_PATH_DENSE_RATIO_LONG : PB_PATH_DENSE_RATIO);
  pb::PlanSpec front = sp.dense;
  front.merged = 1;
  // What the whole rounds leave of the dense class runs one series per wave on the matrix pipe instead of the vector pipe
  // (fista_mfma_row.h) where that kernel has the shape: a plain solve of 129 .. 320 scans with up to 33 taps from the host,
  // the one-wave matrix-pipe form as the call's main form.  The plan is not touched: each one-problem-per-wave candidate's
  // range is cut at the end of the dense class, on the device, into spare words of the workspace.
  const bool row_leftovers = r.path == PATH_PART_SHORT && r.mfma && !(flags & PB_FLAG_VECTOR_LEFTOVERS) && taps_host &&
                             N >= pb::ROW_NMIN && N <= pb::ROW_NMAX && K <= pb::ROW_KMAX && a.stop_mode == PB_STOP_NONE && !a.J &&
                             !a.taps_pp && a.n_done;
  int32_t* rg_split = row_leftovers ? work_dev + wl.split : nullptr;
  int rc = launch_partition(pb::ClassPred{a.lbda_vec, a.lbda, lmax, a.y_rep, ratio, nullptr}, P, work_dev, front, sp.sparse, rg_dense,
                            rg_sparse, rg_ill, "partition", user, rg_split);
  if (rc != PB_OK) return rc;
  Side side;
  if (!one_stream) side.take();
  // ONE list for the call: positions [0, P) of the list array (dense problems first), one plan (plan.h: plan_partitioned)
  const bool only_dense = (flags & PB_FLAG_ONLY_DENSE) != 0, only_sparse = (flags & PB_FLAG_ONLY_SPARSE) != 0;   // (measurement aids)
  rc = solve_list(r, a, lf, user, side, work_dev, rg_dense, only_dense ? 1 : (only_sparse ? 2 : 0), false,
                  (only_dense || only_sparse) ? nullptr : rg_split, taps_host);
  if (rc != PB_OK || only_dense || only_sparse) return rc;
  if (ill_exact || ill_generic) {                // (its workgroups stride over the list, which is empty for ordinary data)
    pb::FistaArgs b = a;
    b.perm = work_dev;
    b.perm_side = 1;
    b.range = rg_ill;
    if (ill_exact) {
      b.grid_slots = P;
      if (ill_exact->fn(b, taps_host, K, a.J != nullptr, a.stop_mode, user) != 0)
        return fail(PB_ERR_INVALID, "%s: float64 kernel rejected the launch (ill-conditioned series)", lf.name);
    } else {
      launch_generic(b, taps_dev, K, a.wind, a.J != nullptr, false, P < 2048 ? P : 2048, user);
    }
    rc = check_launch("float64 kernel (ill-conditioned series)");
    if (rc != PB_OK) return rc;
  }
  // what the guards / certificates handed back (n_done = -1): compacted, then the exact vector forms at full occupancy
  const pb::PlanSpec none{0, 0, 0, 0, 1, 0, 0, sp.dense.slots};
  rc = launch_partition(pb::ClassPred{nullptr, 0.0, nullptr, 1, 0.0, a.n_done}, P, work_dev, sp.flagged, none, rg_flag, nullptr, nullptr,
                        "partition(handed back)", user);
  if (rc != PB_OK) return rc;
  side.ss = nullptr;                             // (one stream: a few per cent of the batch at most)
  return solve_list(r, a, lf, user, side, work_dev, rg_flag, 3, true);
}

// z = L w and x = h * z of every row (one HRF for all: ldt = 0; pp: one per problem)
int outputs_impl(const double* w_dev, int64_t ldw, int P, int N, const double* taps_dev, int64_t ldt, int K, double* z_dev,
                 int64_t ldz, double* x_dev, int64_t ldx, void* stream, bool pp, const char* name) {
  if (P < 0 || N < 1 || K < 1 || ldw < N || (pp && ldt < K) || (z_dev && ldz < N) || (x_dev && ldx < N))
    return fail(PB_ERR_INVALID, "%s: bad size", name);
  if (2 * (int64_t)N + K + 8 > LDS_DOUBLES_MAX) return fail(PB_ERR_INVALID, "%s: N=%d K=%d exceeds LDS", name, N, K);
  if (P == 0 || (!z_dev && !x_dev)) return PB_OK;
  if (!w_dev || !taps_dev) return fail(PB_ERR_INVALID, "%s: NULL pointer", name);
  const size_t lds = (size_t)(2 * N + K + 8) * sizeof(double);
  hipLaunchKernelGGL(pb::outputs_kernel, dim3(P), dim3(pb::GEN_THREADS), lds, (hipStream_t)stream,
                     w_dev, ldw, N, taps_dev, ldt, K, z_dev, ldz, x_dev, ldx);
  return check_launch(name);
}

pb::HrfModel hrf_model(double a_peak, double loc_peak, double a_under, double loc_under, double ratio) {
  return pb::HrfModel{a_peak, loc_peak, lgamma(a_peak), a_under, loc_under, lgamma(a_under), ratio,
                      pb::hrf_int_power(a_peak), pb::hrf_int_power(a_under), std::exp(-lgamma(a_peak)),
                      std::exp(-lgamma(a_under))};
}

// the fields every FISTA entry point fills alike (the series, cost trace and per-problem taps are the caller's)
pb::FistaArgs fista_args(int P, int N, int K, int n_iter, int y_rep, int64_t ldy, double* w, int64_t ldw, double step,
                         double lbda, const double* lbda_vec, const double* betas, int stop_mode, double tol,
                         int32_t* n_done, unsigned flags) {
  pb::FistaArgs a;
  a.y = nullptr; a.y64 = nullptr; a.ldy = ldy; a.w = w; a.ldw = ldw; a.lbda_vec = lbda_vec;
  a.betas = betas; a.J = nullptr; a.J64 = nullptr; a.ldj = 0; a.n_done = n_done;
  a.step = step; a.lbda = lbda; a.tol = tol;
  a.y_rep = y_rep; a.P = P; a.N = N; a.n_iter = n_iter; a.stop_mode = stop_mode;
  a.taps_pp = nullptr; a.ldt = 0; a.step_vec = nullptr; a.step_shared = 0; a.K = K; a.p0 = 0;
  a.cold = (flags & PB_FLAG_COLD_START) ? 1 : 0;
  a.rho_guard = (flags & PB_FLAG_NO_RHO_GUARD) ? 0 : 1;
  return a;
}
}  // namespace

extern "C" {

int pb_version(void) { return 100; }

int pb_init(void) {
  std::lock_guard<std::mutex> lock(g_side_mutex);
  if (!side_stream_locked()) return fail(PB_ERR_HIP, "pb_init: no side stream (is a HIP device current?)");
  g_err[0] = 0;
  return PB_OK;
}

const char* pb_last_error(void) { return g_err; }

int pb_fista_has_fast_path(int N, int K) {
  return (N >= 1 && K >= 1 && (pick_fast(N, K) || pick_wide(N, K))) ? 1 : 0;
}

// The queries describe the call they stand for -- one lambda, n_done given, the tolerance below both certificate limits,
// no workspace -- and report its route
int pb_fista_which_kernel(int N, int K, int P, int with_cost_trace, int stop_mode, int wind) {
  if (N < 1 || K < 1 || P < 1) return 0;
  int nm, mf, tf;
  report(route(Call{N, K, P, stop_mode, wind, 0u, with_cost_trace != 0, false, true, 0.0, false, false, true}), N, P, false, false, &nm, &mf, &tf);
  return nm ? mf : tf;                                  // the form that carries most problems
}

int pb_fista_plan(int N, int K, int P, int stop_mode, int wind, int* n_main, int* main_form,
                  int* tail_form) {
  return pb_fista_plan_ex(N, K, P, stop_mode, wind, 0u, n_main, main_form, tail_form);
}

// (no cost trace; of the flags: the pins of the pair form and direct FIRs read as PB_FLAG_NO_MFMA -- the plan without the
// matrix pipe --, PB_FLAG_ONE_LAUNCH, _FORCE_MFMA2 and _ONE_STREAM)
int pb_fista_plan_ex(int N, int K, int P, int stop_mode, int wind, unsigned flags, int* n_main,
                     int* main_form, int* tail_form) {
  int nm = 0, mf = 0, tf = 0;
  if (N >= 1 && K >= 1 && P >= 1) {
    const unsigned fl = ((flags & FLAGS_PAIR_PIN_OR_NO_MFMA) ? PB_FLAG_NO_MFMA : 0u) |
                        (flags & (PB_FLAG_ONE_LAUNCH | PB_FLAG_FORCE_MFMA2 | PB_FLAG_ONE_STREAM));
    const Route r = route(Call{N, K, P, stop_mode, wind, fl, false, false, true, 0.0, false, false, true});
    // (the plan of the vector forms alone is reported as planned without PB_FLAG_ONE_LAUNCH / _ONE_STREAM)
    report(r, N, P, r.mfma && (fl & PB_FLAG_ONE_LAUNCH), r.mfma && (fl & PB_FLAG_ONE_STREAM), &nm, &mf, &tf);
  }
  if (n_main) *n_main = nm;
  if (main_form) *main_form = mf;
  if (tail_form) *tail_form = tf;
  return PB_OK;
}

static int solve_impl(const float* y_dev, int64_t ldy, int y_rep, double* w_dev, int64_t ldw, int P,
                      int N, const double* taps_host, const double* taps_dev, int K, double step,
                      double lbda,
                      const double* lbda_dev, const double* betas_dev, int n_iter, float* J_dev,
                      int64_t ldj, int stop_mode, double tol, int wind, int32_t* n_done_dev,
                      unsigned flags, void* stream, const double* lmax_dev, double dense_ratio,
                      int32_t* work_dev, int64_t work_len) {
  if (P < 0 || N < 1 || K < 1 || n_iter < 0 || y_rep < 1)
    return fail(PB_ERR_INVALID, "pb_fista_solve: bad size (P=%d N=%d K=%d n_iter=%d y_rep=%d)", P,
                N, K, n_iter, y_rep);
  if (P > 0 && (!y_dev || !w_dev || !taps_host || (n_iter > 0 && !betas_dev)))
    return fail(PB_ERR_INVALID, "pb_fista_solve: NULL pointer");
  if (P > (1 << 25)) return fail(PB_ERR_INVALID, "pb_fista_solve: more than 2^25 problems per launch");
  if (ldy < N || ldw < N) return fail(PB_ERR_INVALID, "pb_fista_solve: leading dimension < N");
  if (J_dev && ldj < n_iter) return fail(PB_ERR_INVALID, "pb_fista_solve: ldj < n_iter");
  if (!(step > 0.0)) return fail(PB_ERR_INVALID, "pb_fista_solve: step must be positive");
  // the reference's prox with a negative threshold grows every entry (its lambda search gets there); only
  // pb_fista_solve_d restates that -- these kernels clamp
  if (!lbda_dev && lbda < 0.0) return fail(PB_ERR_INVALID, "pb_fista_solve: negative lbda (float64 entry point only)");
  if (stop_mode < PB_STOP_NONE || stop_mode > PB_STOP_WINDOW)
    return fail(PB_ERR_INVALID, "pb_fista_solve: unknown stop_mode %d", stop_mode);
  if (stop_mode == PB_STOP_WINDOW && wind < 2)
    return fail(PB_ERR_INVALID, "pb_fista_solve: wind must be >= 2");
  if (P == 0) return PB_OK;

  pb::FistaArgs a = fista_args(P, N, K, n_iter, y_rep, ldy, w_dev, ldw, step, lbda, lbda_dev, betas_dev, stop_mode, tol,
                               n_done_dev, flags);
  a.y = y_dev; a.J = J_dev; a.ldj = ldj; a.wind = wind;
#ifdef PB_DEVELOPMENT                            // (development builds only: the series scale of the matrix-pipe form)
  if (const char* yb = getenv("PB_MFMA_YBITS")) {
    const int v = atoi(yb);
    if (v >= 8 && v <= 15) a.ybits = v;
  }
#endif
  if (flags & PB_FLAG_FORCE_MFMA_ROW) {           // every row on fista_mfma_row_kernel alone, in place (tests, measurements)
    if (N < pb::ROW_NMIN || N > pb::ROW_NMAX || K > pb::ROW_KMAX || J_dev || stop_mode != PB_STOP_NONE || !n_done_dev)
      return fail(PB_ERR_INVALID, "pb_fista_solve: PB_FLAG_FORCE_MFMA_ROW serves plain solves of %d .. %d scans with up to %d taps, "
                  "no cost trace, n_done_dev given (N=%d K=%d stop=%d)", pb::ROW_NMIN, pb::ROW_NMAX, pb::ROW_KMAX, N, K, stop_mode);
    if (pb::launch_mfma_row(a, taps_host, K, false, (hipStream_t)stream) != 0)
      return fail(PB_ERR_INVALID, "pb_fista_solve: fista_mfma_row_kernel rejected its launch");
    return check_launch("fista_mfma_row_kernel");
  }
  const int V_series = (P + y_rep - 1) / y_rep;
  // (PB_FLAG_FORCE_MFMA without the caller's lambda_max: "everything on the matrix pipe", unpartitioned)
  const bool workspace = work_dev && work_len >= work_layout(P, V_series).total && !((flags & PB_FLAG_FORCE_MFMA) && !lmax_dev);
  const Route r = route(Call{N, K, P, stop_mode, wind, flags, J_dev != nullptr, lbda_dev != nullptr, n_done_dev != nullptr,
                             tol * (double)n_iter, taps_dev != nullptr, workspace, false});
  const hipStream_t user = (hipStream_t)stream;
  const HostTapsForms lf{r, "pb_fista_solve", taps_host, K, stop_mode, J_dev != nullptr, (flags & PB_FLAG_DIRECT_FIR) != 0};
  if (r.path == PATH_PART_LONG || r.path == PATH_PART_SHORT)
    return run_partition(r, a, lf, user, taps_host, taps_dev, flags, dense_ratio, work_dev);
  if (r.path != PATH_GENERIC) return run_in_place(r, a, lf, user, flags);
  if (flags & PB_FLAG_FORCE_FAST)
    return fail(PB_ERR_INVALID, "pb_fista_solve: no register-resident kernel for N=%d K=%d stop=%d",
                N, K, stop_mode);
  // generic path (any N, K that fit LDS; all stop rules)
  if (!taps_dev) return fail(PB_ERR_INVALID, "pb_fista_solve: taps_dev required for the generic kernel");
  if (gen_lds_doubles(N, K, stop_mode, wind) > LDS_DOUBLES_MAX)
    return fail(PB_ERR_INVALID, "pb_fista_solve: N=%d K=%d wind=%d exceeds LDS", N, K, wind);
  launch_generic(a, taps_dev, K, wind, J_dev != nullptr, false, P, user);
  return check_launch("fista_generic_kernel");
}

int pb_fista_list_plan(int kind, int n, int n_max, int has_pair, int has_wide, int one_stream, int has_mfma2,
                       int beside_chunks, int32_t* ranges, int32_t* bounds) {
  if (kind < 1 || kind > 3 || n < 0 || n_max < n) return fail(PB_ERR_INVALID, "pb_fista_list_plan: bad argument");
  Piece pc[pb::MAX_PIECES];
  int npc = 0;
  const double slots = wave_slots();
  if (n > 0 && kind == 1) npc = pb::plan_pieces_mfma(n, has_pair != 0, has_wide != 0, false, one_stream != 0, has_mfma2 != 0, beside_chunks, slots, pc);
  else if (n > 0 && kind == 2) npc = pb::plan_pieces(n, has_pair != 0, has_wide != 0, false, one_stream != 0, slots, pc);
  else if (kind == 3 && n_max > 0)      // a partitioned call of n_max problems, n of them dense
    npc = pb::plan_partitioned(n, n_max, has_pair != 0, has_wide != 0, one_stream != 0, has_mfma2 != 0, beside_chunks, slots, pc);
  int32_t rg[2 * pb::CAND_COUNT];
  const int rc = pb::plan_to_candidates(pc, npc, rg);
  for (int c = 0; c < pb::CAND_COUNT; ++c) {
    if (ranges) { ranges[2 * c] = rg[2 * c]; ranges[2 * c + 1] = rg[2 * c + 1]; }
    if (bounds) bounds[c] = pb::cand_max_slots(c, n_max, slots);
  }
  if (rc != 0) return fail(PB_ERR_INVALID, "pb_fista_list_plan: a piece of the plan found its candidate launch taken (n=%d)", n);
  g_err[0] = 0;
  return PB_OK;
}

int pb_mfma_sparse_tile(const double* taps_host, int K, int pass, int parity, int row_half, unsigned short* hi,
                        unsigned short* lo, unsigned short* idx, float* c64) {
  if (!taps_host || !hi || !lo || !idx) return fail(PB_ERR_INVALID, "pb_mfma_sparse_tile: NULL pointer");
  if (pass < 0 || pass > 1 || parity < 0 || parity > 1 || row_half < 0 || row_half > 1)
    return fail(PB_ERR_INVALID, "pb_mfma_sparse_tile: pass, parity and row_half are 0 or 1");
  if (K < 1 || K > pb::SPARSE_TILE_KMAX)
    return fail(PB_ERR_INVALID, "pb_mfma_sparse_tile: K=%d outside 1..%d taps (33 taps put three nonzeros in a group of four)", K,
                pb::SPARSE_TILE_KMAX);
  const pb::MfmaTaps tp = pb::make_mfma_taps(taps_host, K);
  if (pb::build_sparse_tile_host(tp, K, pass, parity, row_half, hi, lo, idx) != 0)
    return fail(PB_ERR_INVALID, "pb_mfma_sparse_tile: a group of four holds more than two nonzeros (K=%d)", K);
  if (c64) memcpy(c64, tp.c, 64 * sizeof(float));
  g_err[0] = 0;
  return PB_OK;
}

int64_t pb_fista_work_len(int P, int y_rep) {
  if (P < 0 || y_rep < 1) return 0;
  return work_layout(P, (P + y_rep - 1) / y_rep).total;
}

int pb_fista_solve_ex(const float* y_dev, int64_t ldy, int y_rep, double* w_dev, int64_t ldw, int P,
                      int N, const double* taps_host, const double* taps_dev, int K, double step,
                      double lbda, const double* lbda_dev, const double* betas_dev, int n_iter, float* J_dev,
                      int64_t ldj, int stop_mode, double tol, int wind, int32_t* n_done_dev,
                      unsigned flags, void* stream, const double* lmax_dev, double dense_ratio,
                      int32_t* work_dev, int64_t work_len) {
  return solve_impl(y_dev, ldy, y_rep, w_dev, ldw, P, N, taps_host, taps_dev, K, step, lbda, lbda_dev, betas_dev, n_iter,
                    J_dev, ldj, stop_mode, tol, wind, n_done_dev, flags, stream, lmax_dev, dense_ratio, work_dev, work_len);
}

int pb_fista_solve(const float* y_dev, int64_t ldy, int y_rep, double* w_dev, int64_t ldw, int P,
                   int N, const double* taps_host, const double* taps_dev, int K, double step,
                   double lbda,
                   const double* lbda_dev, const double* betas_dev, int n_iter, float* J_dev,
                   int64_t ldj, int stop_mode, double tol, int wind, int32_t* n_done_dev,
                   unsigned flags, void* stream) {
  // a workspace of the library's own for the partition (grown on demand, one per device and stream; never while the
  // stream is being captured: an allocation cannot be captured -- such calls, and calls that fail to get memory, run
  // without the partition.  pb_fista_solve_ex takes the caller's workspace instead and allocates nothing.)
  int32_t* work = nullptr;
  int64_t len = 0;
  if (P >= PART_MIN_P && N <= 1280 && n_done_dev && !(flags & PB_FLAG_NO_PARTITION) && !stream_is_capturing((hipStream_t)stream))
    work = own_workspace(stream, work_layout(P, (P + (y_rep > 0 ? y_rep : 1) - 1) / (y_rep > 0 ? y_rep : 1)).total, &len);
  return solve_impl(y_dev, ldy, y_rep, w_dev, ldw, P, N, taps_host, taps_dev, K, step, lbda, lbda_dev, betas_dev, n_iter,
                    J_dev, ldj, stop_mode, tol, wind, n_done_dev, flags, stream, nullptr, 0.0, work, len);
}

// ---- the float64 register family (dispatch.h: kF64, pick_f64): four solve and eight search entry points over one
// validation-and-launch function each ----------------------------------------------------------------------------------------
namespace {
// How a solve names a form that the default dispatch does not choose: by a flag, or by its entry point
struct F64Named {
  int form;
  const char* who;               // what names the form ...
  const char* with;              // ... and how the messages of the form's own checks begin
  unsigned excluded;             // the flags that name another form
  const char* excluded_names;
  const char* taps_host_note;    // beside "NULL pointer" of a call with the taps on the host
};
const F64Named kByLongHrfFlag = {F64_LONG_HRF, "PB_FLAG_LONG_HRF", "PB_FLAG_LONG_HRF with ",
                                 PB_FLAG_FORCE_GENERIC | PB_FLAG_FORCE_FAST | PB_FLAG_PP_SPLIT,
                                 "PB_FLAG_FORCE_GENERIC, PB_FLAG_FORCE_FAST and PB_FLAG_PP_SPLIT", " (PB_FLAG_LONG_HRF reads taps_host)"};
const F64Named kByPPSplitFlag = {F64_FOUR_WAVES, "PB_FLAG_PP_SPLIT", "PB_FLAG_PP_SPLIT with ", PB_FLAG_FORCE_GENERIC | PB_FLAG_FORCE_FAST,
                                 "PB_FLAG_FORCE_GENERIC and PB_FLAG_FORCE_FAST", ""};
const F64Named kBySplitLongEntry = {F64_FOUR_WAVES_LONG_HRF, "the entry point", "",
                                    PB_FLAG_FORCE_GENERIC | PB_FLAG_FORCE_FAST | PB_FLAG_PP_SPLIT | PB_FLAG_LONG_HRF,
                                    "PB_FLAG_FORCE_GENERIC, PB_FLAG_FORCE_FAST, PB_FLAG_PP_SPLIT and PB_FLAG_LONG_HRF", ""};

// the words of a form's messages, with its tap limit in them (built where a message needs them only)
struct F64Words { char label[32], form[64], taps_over[32]; };
F64Words f64_words(const F64FormDesc& d) {
  F64Words w;
  snprintf(w.label, sizeof(w.label), d.label, d.k_max);
  snprintf(w.form, sizeof(w.form), "%s %s", w.label, d.noun);
  snprintf(w.taps_over, sizeof(w.taps_over), d.taps_over, d.k_max);
  return w;
}
// check_launch under the kernel's name: <stem><form>[_pp]_kernel[(final solve)]
int check_f64_launch(const char* stem, int form, bool pp, bool final_solve = false) {
  char what[64];
  snprintf(what, sizeof(what), "%s%s%s_kernel%s", stem, kF64[form].kernels, pp ? "_pp" : "", final_solve ? "(final solve)" : "");
  return check_launch(what);
}

// the entry of the form a solve names, or the error of a call that form does not carry (nothing is launched)
int named_f64_entry(const char* name, const F64Named& by, int N, int K, int stop_mode, int wind, unsigned flags, const ExactEntry** e) {
  const F64FormDesc& d = kF64[by.form];
  if (flags & by.excluded)
    return fail(PB_ERR_INVALID, "%s: %s names the %s; it excludes %s", name, by.who, f64_words(d).form, by.excluded_names);
  if (N < d.n_min || N > d.n_max) return fail(PB_ERR_INVALID, "%s: %sN=%d outside %d..%d scans", name, by.with, N, d.n_min, d.n_max);
  if (K > d.k_max) return fail(PB_ERR_INVALID, "%s: %sK=%d %s", name, by.with, K, f64_words(d).taps_over);
  if (stop_mode == PB_STOP_WINDOW && wind != F64_WIND)
    return fail(PB_ERR_INVALID, "%s: %swind=%d (the %s carries wind = %d)", name, by.with, wind, f64_words(d).form, F64_WIND);
  *e = pick_f64(by.form, N, K, stop_mode, wind);
  if (!*e) return fail(PB_ERR_INVALID, "%s: no %s specialisation for N=%d K=%d", name, f64_words(d).label, N, K);
  return PB_OK;
}

// The four float64 solves: `pp` -- one HRF (taps_dev [P][ldt]) and one step (step_dev [P]) per problem instead of taps_host /
// taps_dev and step; `entry_names` -- the form the entry point names, else the flags name one (PB_FLAG_LONG_HRF; with `pp`,
// PB_FLAG_PP_SPLIT), else the default dispatch chooses, with the any-size LDS kernel behind it.  One validation in one order;
// the two argument lists word three checks differently (the leading dimensions, and the step that only one of them has).
int solve_d(const char* name, bool pp, const F64Named* entry_names, const double* y_dev, int64_t ldy, int y_rep, double* w_dev,
            int64_t ldw, int P, int N, const double* taps_host, const double* taps_dev, int64_t ldt, int K, double step,
            const double* step_dev, double lbda, const double* lbda_dev, const double* betas_dev, int n_iter, double* J_dev,
            int64_t ldj, int stop_mode, double tol, int wind, int32_t* n_done_dev, unsigned flags, void* stream) {
  if (P < 0 || N < 1 || K < 1 || n_iter < 0 || y_rep < 1)
    return fail(PB_ERR_INVALID, "%s: bad size (P=%d N=%d K=%d n_iter=%d y_rep=%d)", name, P, N, K, n_iter, y_rep);
  if (pp && ldt < K) return fail(PB_ERR_INVALID, "%s: ldt < K", name);
  if (ldy < N || ldw < N) return fail(PB_ERR_INVALID, pp ? "%s: leading dimension too small (< N)" : "%s: leading dimension < N", name);
  if (J_dev && ldj < n_iter) return fail(PB_ERR_INVALID, pp ? "%s: leading dimension too small (ldj < n_iter)" : "%s: ldj < n_iter", name);
  if (!pp && !(step > 0.0)) return fail(PB_ERR_INVALID, "%s: step must be positive", name);
  if (stop_mode < PB_STOP_NONE || stop_mode > PB_STOP_WINDOW) return fail(PB_ERR_INVALID, "%s: unknown stop_mode %d", name, stop_mode);
  if (stop_mode == PB_STOP_WINDOW && wind < 2) return fail(PB_ERR_INVALID, "%s: wind must be >= 2", name);
  const F64Named* by = entry_names                          ? entry_names
                       : (flags & PB_FLAG_LONG_HRF)         ? &kByLongHrfFlag
                       : (pp && (flags & PB_FLAG_PP_SPLIT)) ? &kByPPSplitFlag
                                                            : nullptr;
  const ExactEntry* e = nullptr;
  int form = F64_ONE_WAVE;
  if (by) {                                                 // opt-in: that form, or an error
    form = by->form;
    const int rc = named_f64_entry(name, *by, N, K, stop_mode, wind, flags, &e);
    if (rc != PB_OK) return rc;
  } else {
    // the register form where the shape has an entry and (taps on the host) the host copy of the taps is given
    if ((pp || taps_host) && !(flags & PB_FLAG_FORCE_GENERIC)) e = pick_f64_default(N, K, stop_mode, wind, !pp, &form);
    // PB_FLAG_FORCE_FAST keeps the meaning it had before the four-wave form existed: the one-problem-per-wave form or an
    // error (callers and tests pin that it fails beyond 640 scans); the four-wave form is reached by the dispatch only
    if ((!e || form != F64_ONE_WAVE) && (flags & PB_FLAG_FORCE_FAST))
      return fail(PB_ERR_INVALID, "%s: no register-resident float64 kernel with one problem per wave for N=%d K=%d", name, N, K);
    if (!e && gen_lds_doubles(N, K, stop_mode, wind) > LDS_DOUBLES_MAX)
      return fail(PB_ERR_INVALID, "%s: N=%d K=%d wind=%d exceeds LDS", name, N, K, wind);
  }
  if (P == 0) return PB_OK;
  // (taps on the host: a register form reads taps_host, the LDS kernel taps_dev)
  if (!y_dev || !w_dev || (pp ? !taps_dev || !step_dev : e ? !taps_host : !taps_dev) || (n_iter > 0 && !betas_dev))
    return fail(PB_ERR_INVALID, "%s: NULL pointer%s", name, (by && !pp) ? by->taps_host_note : "");
  if (P > (1 << 25)) return fail(PB_ERR_INVALID, "%s: more than 2^25 problems per launch", name);
  pb::FistaArgs a = fista_args(P, N, K, n_iter, y_rep, ldy, w_dev, ldw, pp ? 0.0 : step, lbda, lbda_dev, betas_dev, stop_mode, tol,
                               n_done_dev, flags);
  a.y64 = y_dev; a.J64 = J_dev; a.ldj = ldj;
  if (pp) { a.wind = wind; a.taps_pp = taps_dev; a.ldt = ldt; a.step_vec = step_dev; a.step_shared = 0; }
  if (!e) {
    launch_generic(a, taps_dev, K, wind, J_dev != nullptr, true, P, (hipStream_t)stream);
    return check_launch(pp ? "fista_generic_kernel(f64, pp)" : "fista_generic_kernel(f64)");
  }
  if ((pp ? e->fn_pp(a, J_dev != nullptr, stop_mode, (hipStream_t)stream)
          : e->fn(a, taps_host, K, J_dev != nullptr, stop_mode, (hipStream_t)stream)) != 0)
    return fail(PB_ERR_INVALID, "%s: launch rejected", name);
  return check_f64_launch("fista_exact", form, pp);
}
}  // namespace

int pb_fista_long_hrf_supported(int N, int K, int stop_mode, int wind) { return pick_f64(F64_LONG_HRF, N, K, stop_mode, wind) ? 1 : 0; }

int pb_fista_split_long_hrf_supported(int N, int K, int stop_mode, int wind) {
  return pick_f64(F64_FOUR_WAVES_LONG_HRF, N, K, stop_mode, wind) ? 1 : 0;
}

int pb_fista_pp_split_supported(int N, int K, int stop_mode, int wind) { return pick_f64(F64_FOUR_WAVES, N, K, stop_mode, wind) ? 1 : 0; }

int pb_fista_solve_d(const double* y_dev, int64_t ldy, int y_rep, double* w_dev, int64_t ldw,
                     int P, int N, const double* taps_host, const double* taps_dev, int K,
                     double step, double lbda, const double* lbda_dev, const double* betas_dev,
                     int n_iter, double* J_dev, int64_t ldj, int stop_mode, double tol, int wind,
                     int32_t* n_done_dev, unsigned flags, void* stream) {
  return solve_d("pb_fista_solve_d", false, nullptr, y_dev, ldy, y_rep, w_dev, ldw, P, N, taps_host, taps_dev, 0, K, step, nullptr, lbda,
                 lbda_dev, betas_dev, n_iter, J_dev, ldj, stop_mode, tol, wind, n_done_dev, flags, stream);
}

// pb_fista_solve_d with one HRF and one step per problem, both in device memory.  The four-wave form (641 .. 1 280 scans)
// runs only when PB_FLAG_PP_SPLIT names it: without the flag such series run on the LDS kernel with FistaArgs::taps_pp
int pb_fista_solve_pp_d(const double* y_dev, int64_t ldy, int y_rep, double* w_dev, int64_t ldw, int P, int N,
                        const double* taps_dev, int64_t ldt, int K, const double* step_dev, double lbda,
                        const double* lbda_dev, const double* betas_dev, int n_iter, double* J_dev, int64_t ldj,
                        int stop_mode, double tol, int wind, int32_t* n_done_dev, unsigned flags, void* stream) {
  return solve_d("pb_fista_solve_pp_d", true, nullptr, y_dev, ldy, y_rep, w_dev, ldw, P, N, nullptr, taps_dev, ldt, K, 0.0, step_dev, lbda,
                 lbda_dev, betas_dev, n_iter, J_dev, ldj, stop_mode, tol, wind, n_done_dev, flags, stream);
}

// the two on the four-wave form for HRFs of up to 48 taps, or an error: opt-in by name (the parameter list of
// pb_fista_solve_d: only its LDS kernel reads taps_dev)
int pb_fista_solve_split_long_d(const double* y_dev, int64_t ldy, int y_rep, double* w_dev, int64_t ldw, int P, int N,
                                const double* taps_host, const double* taps_dev, int K, double step, double lbda,
                                const double* lbda_dev, const double* betas_dev, int n_iter, double* J_dev, int64_t ldj, int stop_mode, double tol,
                                int wind, int32_t* n_done_dev, unsigned flags, void* stream) {
  return solve_d("pb_fista_solve_split_long_d", false, &kBySplitLongEntry, y_dev, ldy, y_rep, w_dev, ldw, P, N, taps_host, taps_dev, 0, K,
                 step, nullptr, lbda, lbda_dev, betas_dev, n_iter, J_dev, ldj, stop_mode, tol, wind, n_done_dev, flags, stream);
}

int pb_fista_solve_split_long_pp_d(const double* y_dev, int64_t ldy, int y_rep, double* w_dev, int64_t ldw, int P, int N,
                                   const double* taps_dev, int64_t ldt, int K, const double* step_dev, double lbda,
                                   const double* lbda_dev, const double* betas_dev, int n_iter, double* J_dev, int64_t ldj,
                                   int stop_mode, double tol, int wind, int32_t* n_done_dev, unsigned flags, void* stream) {
  return solve_d("pb_fista_solve_split_long_pp_d", true, &kBySplitLongEntry, y_dev, ldy, y_rep, w_dev, ldw, P, N, nullptr, taps_dev, ldt, K,
                 0.0, step_dev, lbda, lbda_dev, betas_dev, n_iter, J_dev, ldj, stop_mode, tol, wind, n_done_dev, flags, stream);
}

// what pb_fista_solve_d / pb_fista_solve_pp_d run for a call shape without flags (every float64 form writes the cost trace)
int pb_fista_which_kernel_d(int N, int K, int with_cost_trace, int stop_mode, int wind) {
  (void)with_cost_trace;
  if (N < 1 || K < 1) return 0;
  int form = F64_ONE_WAVE;
  if (pick_f64_default(N, K, stop_mode, wind, true, &form)) return form == F64_FOUR_WAVES ? 8 : 7;
  return gen_lds_doubles(N, K, stop_mode, wind) <= LDS_DOUBLES_MAX ? 0 : -1;
}

int pb_fista_which_kernel_pp_d(int N, int K, int with_cost_trace, int stop_mode, int wind) {
  (void)with_cost_trace;
  if (N < 1 || K < 1) return 0;
  if (pick_f64_default(N, K, stop_mode, wind, false)) return 9;
  return gen_lds_doubles(N, K, stop_mode, wind) <= LDS_DOUBLES_MAX ? 0 : -1;
}

int64_t pb_auto_lbda_work_len(int V) { return (int64_t)pb::AUTO_STATE * (V > 0 ? V : 0); }

namespace {
int auto_lbda_supported(int form, int N, int K, int wind) {
  return (wind == pb::AUTO_WIND && pick_f64(form, N, K, PB_STOP_WINDOW, wind)) ? 1 : 0;
}

// The eight device-resident lambda searches: the form is the entry point's; `pp` -- one HRF (taps_dev [V][ld_taps]) and one
// step (step_dev [V]) per voxel instead of taps_host and step.  One validation in one order, one launch protocol: chunks of
// outer iterations (the caller's outer_chunk, else the form's: auto_outer_chunk), then the final solve.  The launches with the
// taps on the host receive the arguments as their AutoArgs base.  The argument lists differ where they must: the taps'
// leading dimension exists with `pp` only, where the traces' is not called ldt; the step's sign is checked where it is a number.
int auto_lbda(const char* name, int form, bool pp, const double* y_dev, int64_t ldy, double* w_dev, int64_t ldw, int cold, int V, int N,
              const double* taps_host, const double* taps_dev, int64_t ld_taps, int K, double step, const double* step_dev,
              const double* betas_dev, const double* sigma_dev, int early_stopping, double tol, int wind, int nb_iter,
              int nb_sub_iter, int outer_chunk, double* R_dev, double* G_dev, double* J_dev, int64_t ld_traces, double* alpha_dev,
              double* lbda_dev, int32_t* n_outer_dev, int64_t* n_inner_dev, double* work_dev, int64_t work_len, void* stream) {
  const F64FormDesc& d = kF64[form];
  if (V < 0 || N < 1 || K < 1) return fail(PB_ERR_INVALID, "%s: bad size (V=%d N=%d K=%d)", name, V, N, K);
  if (wind != pb::AUTO_WIND)
    return fail(PB_ERR_INVALID, "%s: wind=%d (the device-resident search carries wind = %d)", name, wind, pb::AUTO_WIND);
  if (N < d.n_min || N > d.n_max)
    return d.n_min > 1 ? fail(PB_ERR_INVALID, "%s: N=%d outside %d..%d scans", name, N, d.n_min, d.n_max)
                       : fail(PB_ERR_INVALID, "%s: N=%d exceeds %d scans", name, N, d.n_max);
  if (K > d.k_max) return fail(PB_ERR_INVALID, "%s: K=%d exceeds %d taps", name, K, d.k_max);
  const ExactEntry* e = pick_f64(form, N, K, PB_STOP_WINDOW, wind);
  if (!e) return fail(PB_ERR_INVALID, "%s: no specialisation for N=%d K=%d", name, N, K);
  if (nb_iter < 1 || nb_sub_iter < 0 || outer_chunk < 0)
    return fail(PB_ERR_INVALID, "%s: nb_iter >= 1, nb_sub_iter >= 0 and outer_chunk >= 0 are required (%d, %d, %d)", name,
                nb_iter, nb_sub_iter, outer_chunk);
  if (ldy < N || ldw < N) return fail(PB_ERR_INVALID, "%s: leading dimension < N", name);
  if (pp && ld_taps < K) return fail(PB_ERR_INVALID, "%s: ldt < K", name);
  if ((R_dev || G_dev || J_dev) && ld_traces < nb_iter)
    return fail(PB_ERR_INVALID, pp ? "%s: leading dimension of the traces < nb_iter" : "%s: ldt < nb_iter", name);
  if (!pp && !(step > 0.0)) return fail(PB_ERR_INVALID, "%s: step must be positive", name);
  if (work_len < pb_auto_lbda_work_len(V))
    return fail(PB_ERR_INVALID, "%s: workspace of %lld float64, %lld needed", name, (long long)work_len,
                (long long)pb_auto_lbda_work_len(V));
  if (V == 0) return PB_OK;
  if (!y_dev || !w_dev || (pp ? !taps_dev || !step_dev : !taps_host) || !sigma_dev || !work_dev || (nb_sub_iter > 0 && !betas_dev))
    return fail(PB_ERR_INVALID, "%s: NULL pointer", name);
  if (V > (1 << 25)) return fail(PB_ERR_INVALID, "%s: more than 2^25 voxels per call", name);
  pb::AutoArgsPP a;
  a.y = y_dev; a.ldy = ldy; a.w = w_dev; a.ldw = ldw; a.V = V; a.N = N;
  a.cold = cold ? 1 : 0; a.nb_sub_iter = nb_sub_iter; a.step = pp ? 0.0 : step; a.tol = tol;
  a.betas = betas_dev; a.sigma = sigma_dev; a.R = R_dev; a.G = G_dev; a.J = J_dev; a.ldt = ld_traces;
  a.alpha_out = alpha_dev; a.lbda_out = lbda_dev; a.n_outer = n_outer_dev; a.n_inner = n_inner_dev; a.work = work_dev;
  a.taps_pp = taps_dev; a.ld_taps = ld_taps; a.step_vec = step_dev; a.K = K;
  auto launch = [&] {
    return pp ? e->fn_auto_pp(a, early_stopping != 0, (hipStream_t)stream)
              : e->fn_auto(a, taps_host, K, early_stopping != 0, (hipStream_t)stream);
  };
  const int chunk = outer_chunk > 0 ? outer_chunk : auto_outer_chunk(form, V, nb_sub_iter);
  for (int i0 = 0; i0 < nb_iter; i0 += chunk) {        // outer iterations [i0, i1) of the voxels still searching
    a.init = i0 == 0; a.i0 = i0; a.i1 = (nb_iter - i0 < chunk) ? nb_iter : i0 + chunk; a.final_solve = 0;
    if (launch() != 0) return fail(PB_ERR_INVALID, "%s: launch rejected", name);
    const int rc = check_f64_launch("auto_lbda", form, pp);
    if (rc != PB_OK) return rc;
  }
  a.init = 0; a.i0 = a.i1 = nb_iter; a.final_solve = 1;   // the last inner solve of every voxel, then the outputs
  if (launch() != 0) return fail(PB_ERR_INVALID, "%s: launch rejected", name);
  return check_f64_launch("auto_lbda", form, pp, true);
}
}  // namespace

int pb_auto_lbda_supported(int N, int K, int wind) { return auto_lbda_supported(F64_ONE_WAVE, N, K, wind); }
int pb_auto_lbda_split_supported(int N, int K, int wind) { return auto_lbda_supported(F64_FOUR_WAVES, N, K, wind); }
int pb_auto_lbda_long_supported(int N, int K, int wind) { return auto_lbda_supported(F64_LONG_HRF, N, K, wind); }
int pb_auto_lbda_split_long_supported(int N, int K, int wind) { return auto_lbda_supported(F64_FOUR_WAVES_LONG_HRF, N, K, wind); }

// the eight entry points: two parameter lists (taps_host, K, step / taps_dev, ldt, K, step_dev), four forms
#define PB_AUTO_LBDA_D(fn, form)                                                                                                \
  int fn(const double* y_dev, int64_t ldy, double* w_dev, int64_t ldw, int cold, int V, int N, const double* taps_host, int K,    \
         double step, const double* betas_dev, const double* sigma_dev, int early_stopping, double tol, int wind, int nb_iter,    \
         int nb_sub_iter, int outer_chunk, double* R_dev, double* G_dev, double* J_dev, int64_t ldt, double* alpha_dev,           \
         double* lbda_dev, int32_t* n_outer_dev, int64_t* n_inner_dev, double* work_dev, int64_t work_len, void* stream) {        \
    return auto_lbda(#fn, form, false, y_dev, ldy, w_dev, ldw, cold, V, N, taps_host, nullptr, 0, K, step, nullptr, betas_dev,    \
                     sigma_dev, early_stopping, tol, wind, nb_iter, nb_sub_iter, outer_chunk, R_dev, G_dev, J_dev, ldt, alpha_dev, \
                     lbda_dev, n_outer_dev, n_inner_dev, work_dev, work_len, stream);                                             \
  }
#define PB_AUTO_LBDA_PP_D(fn, form)                                                                                             \
  int fn(const double* y_dev, int64_t ldy, double* w_dev, int64_t ldw, int cold, int V, int N, const double* taps_dev,            \
         int64_t ldt, int K, const double* step_dev, const double* betas_dev, const double* sigma_dev, int early_stopping,        \
         double tol, int wind, int nb_iter, int nb_sub_iter, int outer_chunk, double* R_dev, double* G_dev, double* J_dev,        \
         int64_t ldtr, double* alpha_dev, double* lbda_dev, int32_t* n_outer_dev, int64_t* n_inner_dev, double* work_dev,         \
         int64_t work_len, void* stream) {                                                                                        \
    return auto_lbda(#fn, form, true, y_dev, ldy, w_dev, ldw, cold, V, N, nullptr, taps_dev, ldt, K, 0.0, step_dev, betas_dev,    \
                     sigma_dev, early_stopping, tol, wind, nb_iter, nb_sub_iter, outer_chunk, R_dev, G_dev, J_dev, ldtr,          \
                     alpha_dev, lbda_dev, n_outer_dev, n_inner_dev, work_dev, work_len, stream);                                  \
  }
PB_AUTO_LBDA_D(pb_auto_lbda_d, F64_ONE_WAVE)
PB_AUTO_LBDA_D(pb_auto_lbda_split_d, F64_FOUR_WAVES)
PB_AUTO_LBDA_D(pb_auto_lbda_long_d, F64_LONG_HRF)
PB_AUTO_LBDA_D(pb_auto_lbda_split_long_d, F64_FOUR_WAVES_LONG_HRF)
PB_AUTO_LBDA_PP_D(pb_auto_lbda_pp_d, F64_ONE_WAVE)
PB_AUTO_LBDA_PP_D(pb_auto_lbda_split_pp_d, F64_FOUR_WAVES)
PB_AUTO_LBDA_PP_D(pb_auto_lbda_long_pp_d, F64_LONG_HRF)
PB_AUTO_LBDA_PP_D(pb_auto_lbda_split_long_pp_d, F64_FOUR_WAVES_LONG_HRF)
#undef PB_AUTO_LBDA_D
#undef PB_AUTO_LBDA_PP_D

int pb_mad_daub_noise_est(const float* y_dev, int64_t ldy, int V, int N, double c, double* sigma_dev, void* stream) {
  return mad_daub_impl<float>(y_dev, ldy, V, N, c, sigma_dev, stream, "pb_mad_daub_noise_est");
}
int pb_mad_daub_noise_est_d(const double* y_dev, int64_t ldy, int V, int N, double c, double* sigma_dev, void* stream) {
  return mad_daub_impl<double>(y_dev, ldy, V, N, c, sigma_dev, stream, "pb_mad_daub_noise_est_d");
}

int pb_fista_solve_backtrack_d(const double* y_dev, int64_t ldy, int y_rep, double* w_dev, int64_t ldw, int P, int N,
                               const double* taps_dev, int K, double step0, double eta, int max_halvings_per_iter,
                               double lbda, const double* lbda_dev, const double* betas_dev, int n_iter,
                               int32_t* n_done_dev, double* step_out_dev, int32_t* halvings_out_dev, unsigned flags, void* stream) {
  if (P < 0 || N < 1 || K < 1 || n_iter < 0 || y_rep < 1)
    return fail(PB_ERR_INVALID, "pb_fista_solve_backtrack_d: bad size (P=%d N=%d K=%d n_iter=%d y_rep=%d)", P, N, K, n_iter, y_rep);
  if (ldy < N || ldw < N) return fail(PB_ERR_INVALID, "pb_fista_solve_backtrack_d: leading dimension < N");
  if (!(step0 > 0.0) || !(eta > 0.0 && eta < 1.0) || max_halvings_per_iter < 0)
    return fail(PB_ERR_INVALID, "pb_fista_solve_backtrack_d: step0 > 0, 0 < eta < 1 and max_halvings_per_iter >= 0 are required");
  const int64_t nd = 5 * (int64_t)N + K + 2 * pb::GEN_WAVES;
  if (nd > LDS_DOUBLES_MAX) return fail(PB_ERR_INVALID, "pb_fista_solve_backtrack_d: N=%d K=%d exceeds LDS", N, K);
  if (P == 0) return PB_OK;
  if (!y_dev || !w_dev || !taps_dev || (n_iter > 0 && !betas_dev)) return fail(PB_ERR_INVALID, "pb_fista_solve_backtrack_d: NULL pointer");
  pb::FistaArgs a = fista_args(P, N, K, n_iter, y_rep, ldy, w_dev, ldw, step0, lbda, lbda_dev, betas_dev, PB_STOP_NONE, 0.0,
                               n_done_dev, flags & PB_FLAG_COLD_START);     // (no matrix-pipe guard here)
  a.y64 = y_dev;
  hipLaunchKernelGGL(pb::fista_backtrack_kernel, dim3(P), dim3(pb::GEN_THREADS), (size_t)nd * sizeof(double), (hipStream_t)stream,
                     a, taps_dev, K, eta, max_halvings_per_iter, step_out_dev, halvings_out_dev);
  return check_launch("fista_backtrack_kernel");
}

int pb_fista_outputs(const double* w_dev, int64_t ldw, int P, int N, const double* taps_dev, int K,
                     double* z_dev, int64_t ldz, double* x_dev, int64_t ldx, void* stream) {
  return outputs_impl(w_dev, ldw, P, N, taps_dev, 0, K, z_dev, ldz, x_dev, ldx, stream, false, "pb_fista_outputs");
}

int pb_fista_outputs_pp(const double* w_dev, int64_t ldw, int P, int N, const double* taps_dev,
                        int64_t ldt, int K, double* z_dev, int64_t ldz, double* x_dev, int64_t ldx,
                        void* stream) {
  return outputs_impl(w_dev, ldw, P, N, taps_dev, ldt, K, z_dev, ldz, x_dev, ldx, stream, true, "pb_fista_outputs_pp");
}

int pb_spm_hrf(const double* deltas_dev, int M, const double* t_dev, int K, double a_peak,
               double loc_peak, double a_under, double loc_under, double ratio, double* out_dev,
               void* stream) {
  if (M < 0 || K < 1 || !(a_peak > 0.0) || !(a_under > 0.0))
    return fail(PB_ERR_INVALID, "pb_spm_hrf: bad argument");
  if (M == 0) return PB_OK;
  if (!deltas_dev || !t_dev || !out_dev) return fail(PB_ERR_INVALID, "pb_spm_hrf: NULL pointer");
  const int64_t total = (int64_t)M * K;
  const unsigned blocks = (unsigned)((total + pb::GEN_THREADS - 1) / pb::GEN_THREADS);
  hipLaunchKernelGGL(pb::spm_hrf_kernel, dim3(blocks), dim3(pb::GEN_THREADS), 0, (hipStream_t)stream,
                     deltas_dev, M, t_dev, K, a_peak, loc_peak, lgamma(a_peak), a_under, loc_under,
                     lgamma(a_under), ratio, out_dev);
  return check_launch("spm_hrf_kernel");
}


int pb_fista_stats(const double* w_dev, int64_t ldw, const float* y_dev, int64_t ldy, int y_rep,
                   int P, int N, const double* taps_dev, int K, double* r2_dev, double* l1_dev,
                   void* stream) {
  return stats_impl<float>(w_dev, ldw, y_dev, ldy, y_rep, P, N, taps_dev, K, r2_dev, l1_dev, stream,
                           "pb_fista_stats");
}
int pb_fista_stats_d(const double* w_dev, int64_t ldw, const double* y_dev, int64_t ldy, int y_rep,
                     int P, int N, const double* taps_dev, int K, double* r2_dev, double* l1_dev,
                     void* stream) {
  return stats_impl<double>(w_dev, ldw, y_dev, ldy, y_rep, P, N, taps_dev, K, r2_dev, l1_dev, stream,
                            "pb_fista_stats_d");
}

int pb_spectral_radius(const double* x0_dev, int N, const double* taps_dev, int K, int nb_iter,
                       double tol, double* out_dev, void* stream) {
  if (N < 1 || K < 1 || nb_iter < 0) return fail(PB_ERR_INVALID, "pb_spectral_radius: bad size");
  if (!x0_dev || !taps_dev || !out_dev) return fail(PB_ERR_INVALID, "pb_spectral_radius: NULL pointer");
  if (3 * (int64_t)N + K + 8 > LDS_DOUBLES_MAX)
    return fail(PB_ERR_INVALID, "pb_spectral_radius: N=%d K=%d exceeds LDS", N, K);
  const size_t lds = (size_t)(3 * N + K + 8) * sizeof(double);
  hipLaunchKernelGGL(pb::power_iter_kernel, dim3(1), dim3(pb::GEN_THREADS), lds, (hipStream_t)stream,
                     x0_dev, (int64_t)0, N, taps_dev, (int64_t)0, K, nb_iter, tol, out_dev);
  return check_launch("power_iter_kernel");
}

int pb_spectral_radius_pp(const double* x0_dev, int64_t ldx, int V, int N, const double* taps_dev, int64_t ldt, int K,
                          int nb_iter, double tol, double* out_dev, void* stream) {
  if (V < 0 || N < 1 || K < 1 || nb_iter < 0)
    return fail(PB_ERR_INVALID, "pb_spectral_radius_pp: bad size (V=%d N=%d K=%d nb_iter=%d)", V, N, K, nb_iter);
  if (ldt < K) return fail(PB_ERR_INVALID, "pb_spectral_radius_pp: ldt < K");
  if (ldx < N) return fail(PB_ERR_INVALID, "pb_spectral_radius_pp: leading dimension too small (ldx < N)");
  if (3 * (int64_t)N + K + 8 > LDS_DOUBLES_MAX)
    return fail(PB_ERR_INVALID, "pb_spectral_radius_pp: N=%d K=%d exceeds LDS", N, K);
  if (V == 0) return PB_OK;
  if (!x0_dev || !taps_dev || !out_dev) return fail(PB_ERR_INVALID, "pb_spectral_radius_pp: NULL pointer");
  const size_t lds = (size_t)(3 * N + K + 8) * sizeof(double);
  hipLaunchKernelGGL(pb::power_iter_kernel, dim3(V), dim3(pb::GEN_THREADS), lds, (hipStream_t)stream,
                     x0_dev, ldx, N, taps_dev, ldt, K, nb_iter, tol, out_dev);
  return check_launch("power_iter_kernel(pp)");
}

int pb_integ_op(const double* x, int64_t ldx, double* out, int64_t ldo, int V, int N, void* st) {
  return launch_op<pb::OP_INTEG>(x, ldx, out, ldo, V, N, N, nullptr, 0, st, "pb_integ_op");
}
int pb_integ_adj(const double* x, int64_t ldx, double* out, int64_t ldo, int V, int N, void* st) {
  return launch_op<pb::OP_INTEG_ADJ>(x, ldx, out, ldo, V, N, N, nullptr, 0, st, "pb_integ_adj");
}
int pb_conv(const double* x, int64_t ldx, double* out, int64_t ldo, int V, int n_in, int n_out,
            const double* taps, int K, void* st) {
  return launch_op<pb::OP_CONV>(x, ldx, out, ldo, V, n_in, n_out, taps, K, st, "pb_conv");
}
int pb_corr(const double* r, int64_t ldr, double* out, int64_t ldo, int V, int n_in, int n_out,
            const double* taps, int K, void* st) {
  // r has n_out samples (the range of the Toeplitz matrix), the result n_in
  return launch_op<pb::OP_CORR>(r, ldr, out, ldo, V, n_out, n_in, taps, K, st, "pb_corr");
}
int pb_op_forward(const double* x, int64_t ldx, double* out, int64_t ldo, int V, int n_in, int n_out,
                  const double* taps, int K, void* st) {
  return launch_op<pb::OP_FWD>(x, ldx, out, ldo, V, n_in, n_out, taps, K, st, "pb_op_forward");
}
int pb_op_adjoint(const double* r, int64_t ldr, double* out, int64_t ldo, int V, int n_in, int n_out,
                  const double* taps, int K, void* st) {
  return launch_op<pb::OP_ADJ>(r, ldr, out, ldo, V, n_out, n_in, taps, K, st, "pb_op_adjoint");
}
int pb_spectral_conv(const double* x, int64_t ldx, double* out, int64_t ldo, int V, int N, const int32_t* map,
                     int L, int pad_left, const double* filt, int T, void* st) {
  return launch_spectral<false>(x, ldx, out, ldo, V, N, map, L, pad_left, filt, T, st, "pb_spectral_conv");
}
int pb_spectral_corr(const double* x, int64_t ldx, double* out, int64_t ldo, int V, int N, const int32_t* map,
                     int L, int pad_left, const double* filt, int T, void* st) {
  return launch_spectral<true>(x, ldx, out, ldo, V, N, map, L, pad_left, filt, T, st, "pb_spectral_corr");
}

int pb_hrf_cost(const double* z_dev, int64_t ldz, const float* y_dev, int64_t ldy, int V, int N,
                const double* taps_dev, int K, int n_hrf, double* cost_dev, void* stream) {
  return hrf_cost_impl<float>(z_dev, ldz, y_dev, ldy, V, N, taps_dev, K, n_hrf, cost_dev, 0, stream,
                              "pb_hrf_cost");
}
int pb_hrf_cost_d(const double* z_dev, int64_t ldz, const double* y_dev, int64_t ldy, int V, int N,
                  const double* taps_dev, int K, int n_hrf, double* cost_dev, void* stream) {
  return hrf_cost_impl<double>(z_dev, ldz, y_dev, ldy, V, N, taps_dev, K, n_hrf, cost_dev, 0, stream,
                               "pb_hrf_cost_d");
}
int pb_hrf_cost_pv(const double* z_dev, int64_t ldz, const float* y_dev, int64_t ldy, int V, int N,
                   const double* taps_dev, int K, int n_hrf, double* cost_dev, void* stream) {
  return hrf_cost_impl<float>(z_dev, ldz, y_dev, ldy, V, N, taps_dev, K, n_hrf, cost_dev, 1, stream,
                              "pb_hrf_cost_pv");
}
int pb_hrf_cost_pv_d(const double* z_dev, int64_t ldz, const double* y_dev, int64_t ldy, int V,
                     int N, const double* taps_dev, int K, int n_hrf, double* cost_dev,
                     void* stream) {
  return hrf_cost_impl<double>(z_dev, ldz, y_dev, ldy, V, N, taps_dev, K, n_hrf, cost_dev, 1, stream,
                               "pb_hrf_cost_pv_d");
}

int pb_gram_frobenius(const double* taps_dev, int64_t ldt, int P, int K, int N, double* out_dev,
                      void* stream) {
  if (P < 0 || K < 1 || N < 1 || (P > 1 && ldt < K))
    return fail(PB_ERR_INVALID, "pb_gram_frobenius: bad size");
  if ((int64_t)N + 8 > LDS_DOUBLES_MAX) return fail(PB_ERR_INVALID, "pb_gram_frobenius: exceeds LDS");
  if (P == 0) return PB_OK;
  if (!taps_dev || !out_dev) return fail(PB_ERR_INVALID, "pb_gram_frobenius: NULL pointer");
  if (K <= N && K <= 1024) {                     // the FIR form: O(K^2 + N) per HRF
    hipLaunchKernelGGL(pb::gram_frobenius_fir_kernel, dim3(P), dim3(64), (size_t)3 * K * sizeof(double),
                       (hipStream_t)stream, taps_dev, ldt, K, N, out_dev);
    return check_launch("gram_frobenius_fir_kernel");
  }
  const size_t lds = (size_t)(N + 8) * sizeof(double);
  hipLaunchKernelGGL(pb::gram_frobenius_kernel, dim3(P), dim3(pb::GEN_THREADS), lds,
                     (hipStream_t)stream, taps_dev, ldt, K < N ? K : N, N, out_dev);
  return check_launch("gram_frobenius_kernel");
}

int pb_lambda_max(const float* y_dev, int64_t ldy, int V, int N, const double* taps_dev, int K,
                  double* out_dev, void* stream) {
  return lambda_max_impl<float>(y_dev, ldy, V, N, taps_dev, K, out_dev, stream, "pb_lambda_max");
}
int pb_lambda_max_d(const double* y_dev, int64_t ldy, int V, int N, const double* taps_dev, int K,
                    double* out_dev, void* stream) {
  return lambda_max_impl<double>(y_dev, ldy, V, N, taps_dev, K, out_dev, stream, "pb_lambda_max_d");
}

int pb_inf_norm(const double* x_dev, int64_t ldx, double* out_dev, int64_t ldo, int V, int64_t n,
                void* stream) {
  if (V < 0 || n < 1 || (V > 1 && (ldx < n || ldo < n)))
    return fail(PB_ERR_INVALID, "pb_inf_norm: bad size");
  if (V == 0) return PB_OK;
  if (!x_dev || !out_dev) return fail(PB_ERR_INVALID, "pb_inf_norm: NULL pointer");
  hipLaunchKernelGGL(pb::inf_norm_kernel, dim3(V), dim3(pb::GEN_THREADS), 0, (hipStream_t)stream,
                     x_dev, ldx, out_dev, ldo, n);
  return check_launch("pb_inf_norm");
}

int64_t pb_hrf_normal_eq_len(int K) { return K >= 1 ? (int64_t)pb::ne_len(K) : 0; }

int pb_hrf_normal_eq(const double* z_dev, int64_t ldz, const float* y_dev, int64_t ldy, int V,
                     int N, int K, int per_voxel, double* work_dev, int64_t work_len,
                     double* out_dev, void* stream) {
  return normal_eq_impl<float>(z_dev, ldz, y_dev, ldy, V, N, K, per_voxel, work_dev, work_len,
                               out_dev, stream, "pb_hrf_normal_eq");
}
int pb_hrf_normal_eq_d(const double* z_dev, int64_t ldz, const double* y_dev, int64_t ldy, int V,
                       int N, int K, int per_voxel, double* work_dev, int64_t work_len,
                       double* out_dev, void* stream) {
  return normal_eq_impl<double>(z_dev, ldz, y_dev, ldy, V, N, K, per_voxel, work_dev, work_len,
                                out_dev, stream, "pb_hrf_normal_eq_d");
}

// (more than 64 KB of dynamic LDS -- K >= 63 -- has to be asked for, per kernel and device, as in launch_mfma4)
static void theta_fit_lds(int64_t nd) {
  if (nd * (int64_t)sizeof(double) > 65536)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(pb::theta_fit_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(nd * sizeof(double)));
}

int pb_theta_fit(const double* ne_dev, int64_t ldne, int M, int K, const double* t_dev,
                 double a_peak, double loc_peak, double a_under, double loc_under, double ratio,
                 double lo, double hi, int n_refine, double* theta_dev, double* cost_dev,
                 double* taps_dev, int64_t ldt, void* stream) {
  if (M < 0 || K < 1 || K > 127 || n_refine < 1 || !(a_peak > 0.0) || !(a_under > 0.0) ||
      !(lo <= hi) || (M > 1 && ldne < pb::ne_len(K)) || (taps_dev && M > 1 && ldt < K))
    return fail(PB_ERR_INVALID, "pb_theta_fit: bad argument");
  const int64_t nd = pb::theta_fit_lds_doubles(K);      // (K > 111: the first scan in groups of 16 candidates)
  if (nd > LDS_DOUBLES_MAX) return fail(PB_ERR_INVALID, "pb_theta_fit: K=%d exceeds LDS", K);
  if (M == 0) return PB_OK;
  if (!ne_dev || !t_dev || !theta_dev || !cost_dev)
    return fail(PB_ERR_INVALID, "pb_theta_fit: NULL pointer");
  const pb::HrfModel hm = hrf_model(a_peak, loc_peak, a_under, loc_under, ratio);
  theta_fit_lds(nd);
  hipLaunchKernelGGL(pb::theta_fit_kernel, dim3(M), dim3(256), (size_t)nd * sizeof(double),
                     (hipStream_t)stream, ne_dev, ldne, M, K, t_dev, hm, lo, hi, n_refine, theta_dev,
                     cost_dev, taps_dev, ldt, 0, (double*)nullptr, 0.0, (double*)nullptr);
  return check_launch("pb_theta_fit");
}

int pb_theta_fit_step(const double* msg_dev, int K, const double* t_dev, double a_peak,
                      double loc_peak, double a_under, double loc_under, double ratio, double lo,
                      double hi, int n_refine, int N, double lbda, double* theta_dev,
                      double* cost_dev, double* taps_dev, double* step_dev, double* jcost_dev,
                      void* stream) {
  if (K < 1 || K > 127 || N < K || n_refine < 1 || !(a_peak > 0.0) || !(a_under > 0.0) || !(lo <= hi))
    return fail(PB_ERR_INVALID, "pb_theta_fit_step: bad argument");
  const int64_t nd = pb::theta_fit_lds_doubles(K);      // (K > 111: the first scan in groups of 16 candidates)
  if (nd > LDS_DOUBLES_MAX) return fail(PB_ERR_INVALID, "pb_theta_fit_step: K=%d exceeds LDS", K);
  if (!msg_dev || !t_dev || !theta_dev || !cost_dev || !taps_dev || !step_dev || !jcost_dev)
    return fail(PB_ERR_INVALID, "pb_theta_fit_step: NULL pointer");
  const pb::HrfModel hm = hrf_model(a_peak, loc_peak, a_under, loc_under, ratio);
  theta_fit_lds(nd);
  hipLaunchKernelGGL(pb::theta_fit_kernel, dim3(1), dim3(256), (size_t)nd * sizeof(double),
                     (hipStream_t)stream, msg_dev, (int64_t)pb::ne_len(K) + 1, 1, K, t_dev, hm, lo, hi,
                     n_refine, theta_dev, cost_dev, taps_dev, (int64_t)K, N, step_dev, lbda, jcost_dev);
  return check_launch("pb_theta_fit_step");
}

int pb_hrf_normal_eq_w(const double* w_dev, int64_t ldw, const float* y_dev, int64_t ldy, int V,
                       int N, int K, double* work_dev, int64_t work_len, double* out_dev,
                       void* stream) {
  if (V < 0 || N < 1 || K < 1 || K > 127 || ldw < N || ldy < N)
    return fail(PB_ERR_INVALID, "pb_hrf_normal_eq_w: bad size (V=%d N=%d K=%d)", V, N, K);
  const int ne = pb::ne_len(K) + 1;
  const int64_t nd = (int64_t)pb::ne_sum_lds_doubles(N, K);
  if (nd > LDS_DOUBLES_MAX) return fail(PB_ERR_INVALID, "pb_hrf_normal_eq_w: N=%d K=%d exceeds LDS", N, K);
  if (!out_dev) return fail(PB_ERR_INVALID, "pb_hrf_normal_eq_w: NULL output");
  int blocks = V < NE_MAX_BLOCKS ? V : NE_MAX_BLOCKS;
  if (work_len / ne < blocks) blocks = (int)(work_len / ne);
  if (V > 0) {
    if (blocks < 1 || !work_dev)
      return fail(PB_ERR_INVALID, "pb_hrf_normal_eq_w: work buffer must hold at least %d doubles", ne);
    if (!w_dev || !y_dev) return fail(PB_ERR_INVALID, "pb_hrf_normal_eq_w: NULL pointer");
    if (ne_wave_form(N, K)) {
      blocks = ne_wave_blocks(V, blocks);
      const size_t lds = (size_t)pb::ne_wave_lds_doubles(N, K) * sizeof(double);
      if (K * K <= 64 * 12 && N <= 64 * 5)
        hipLaunchKernelGGL((pb::normal_eq_wave_kernel<float, true, 12, 5>), dim3(blocks), dim3(pb::NE_THREADS), lds,
                           (hipStream_t)stream, w_dev, ldw, y_dev, ldy, V, N, K, work_dev);
      else
        hipLaunchKernelGGL((pb::normal_eq_wave_kernel<float, true>), dim3(blocks), dim3(pb::NE_THREADS), lds,
                           (hipStream_t)stream, w_dev, ldw, y_dev, ldy, V, N, K, work_dev);
    } else {
      hipLaunchKernelGGL((pb::normal_eq_sum_kernel<float, true>), dim3(blocks), dim3(pb::NE_THREADS),
                         (size_t)nd * sizeof(double), (hipStream_t)stream, w_dev, ldw, y_dev, ldy, V, N, K,
                         work_dev);
    }
  } else {
    blocks = 0;
  }
  hipLaunchKernelGGL(pb::normal_eq_reduce_kernel, dim3(ne), dim3(pb::NE_THREADS), 0,
                     (hipStream_t)stream, work_dev, blocks, ne, out_dev);
  return check_launch("pb_hrf_normal_eq_w");
}


int pb_fista_solve_pp(const float* y_dev, int64_t ldy, double* w_dev, int64_t ldw, int P, int N,
                      const double* taps_dev, int64_t ldt, int K, const double* step_dev,
                      double lbda, const double* lbda_dev, const double* betas_dev, int n_iter,
                      int stop_mode, double tol, int32_t* n_done_dev, unsigned flags, void* stream) {
  if (P < 0 || N < 1 || K < 1 || n_iter < 0)
    return fail(PB_ERR_INVALID, "pb_fista_solve_pp: bad size (P=%d N=%d K=%d n_iter=%d)", P, N, K, n_iter);
  if (P > (1 << 25)) return fail(PB_ERR_INVALID, "pb_fista_solve_pp: more than 2^25 problems per launch");
  if (ldy < N || ldw < N || (ldt != 0 && ldt < K))
    return fail(PB_ERR_INVALID, "pb_fista_solve_pp: leading dimension too small");
  if (P == 0) return PB_OK;
  if (!y_dev || !w_dev || !taps_dev || !step_dev || (n_iter > 0 && !betas_dev))
    return fail(PB_ERR_INVALID, "pb_fista_solve_pp: NULL pointer");
  if (stop_mode != PB_STOP_NONE && stop_mode != PB_STOP_LOOPS)
    return fail(PB_ERR_INVALID, "pb_fista_solve_pp: stop_mode must be PB_STOP_NONE or PB_STOP_LOOPS");

  pb::FistaArgs a = fista_args(P, N, K, n_iter, 1, ldy, w_dev, ldw, 0.0, lbda, lbda_dev, betas_dev, stop_mode, tol, n_done_dev, flags);
  a.y = y_dev; a.taps_pp = taps_dev; a.ldt = ldt; a.step_vec = step_dev; a.step_shared = (ldt == 0);
  const hipStream_t user = (hipStream_t)stream;
  const Route r = route_pp(N, K, P, ldt == 0, stop_mode, n_done_dev != nullptr, flags);
  if (r.path != PATH_GENERIC) return run_in_place(r, a, DeviceTapsForms{r, "pb_fista_solve_pp", K, stop_mode}, user, flags);
  if (flags & PB_FLAG_FORCE_FAST)
    return fail(PB_ERR_INVALID, "pb_fista_solve_pp: no register-resident kernel for N=%d K=%d", N, K);
  if (gen_lds_doubles(N, K, stop_mode, 0) > LDS_DOUBLES_MAX) return fail(PB_ERR_INVALID, "pb_fista_solve_pp: N=%d K=%d exceeds LDS", N, K);
  launch_generic(a, taps_dev, K, 0, false, false, P, user);
  return check_launch("fista_generic_kernel(pp)");
}

// ---- one HRF per parcel (rows contiguous by parcel; plan.h: the unit table, grouped.h: its device side) ----
}  // extern "C"
namespace {
constexpr int NE_GROUPED_UNITS = 1024, NE_GROUPED_MIN_ROWS = 16;     // normal equations: ~1 024 workgroups, 16 rows at least each

struct GroupedWork { int64_t taps, steps, first, table, total; };    // offsets in int32 words (the float64 parts first)
GroupedWork grouped_work(int P, int G, int K) {
  GroupedWork w;
  w.taps = 0;
  w.steps = w.taps + 2 * (int64_t)P * K;
  w.first = w.steps + 2 * (int64_t)P;
  w.table = w.first + (((int64_t)G + 2) & ~(int64_t)1);
  w.total = w.table + pb::GROUPED_WORDS * pb::grouped_max_units(P, G, pb::GROUPED_WAVE_ROWS);
  return w;
}
// first [G + 1] and table [3 * units] of a grouped call from the offsets in device memory (grouped.h)
void launch_grouped_table(const int32_t* offsets_dev, int G, int P, int per, int u_max, int32_t* first, int32_t* table, hipStream_t st) {
  hipLaunchKernelGGL(pb::grouped_first_kernel, dim3(1), dim3(pb::GROUPED_TABLE_THREADS), 0, st, offsets_dev, G, P, per, u_max, first);
  if (u_max > 0)
    hipLaunchKernelGGL(pb::grouped_units_kernel, dim3((unsigned)((u_max + pb::GROUPED_TABLE_THREADS - 1) / pb::GROUPED_TABLE_THREADS)),
                       dim3(pb::GROUPED_TABLE_THREADS), 0, st, offsets_dev, G, P, per, first, table);
}
int ne_grouped_rows(int V) {
  const int per = (V + NE_GROUPED_UNITS - 1) / NE_GROUPED_UNITS;
  return per < NE_GROUPED_MIN_ROWS ? NE_GROUPED_MIN_ROWS : per;
}
// float64 work buffer of the grouped normal equations: first [G + 1] and the unit table (int32), then the units' sets
struct NeGroupedWork { int64_t max_units, part, total; };            // `part`, `total` in doubles
NeGroupedWork ne_grouped_work(int V, int G, int K) {
  NeGroupedWork w;
  w.max_units = pb::grouped_max_units(V, G, ne_grouped_rows(V));
  w.part = ((int64_t)G + 2 + pb::GROUPED_WORDS * w.max_units + 1) / 2;
  w.total = w.part + w.max_units * (pb::ne_len(K) + 1);
  return w;
}
}  // namespace
extern "C" {

int64_t pb_fista_grouped_work_len(int P, int G, int K) { return (P >= 0 && G >= 0 && K >= 1) ? grouped_work(P, G, K).total : 0; }

int pb_fista_grouped_plan(const int32_t* offsets_host, int G, int P, int per, int32_t* table_out, int32_t* first_out) {
  if (P < 0 || per < 1 || !pb::grouped_offsets_ok(offsets_host, G, P)) return -1;
  return pb::grouped_table(offsets_host, G, P, per, table_out, first_out);
}

int pb_fista_grouped_waves(const int32_t* offsets_host, int G, int P) {
  return pb_fista_grouped_plan(offsets_host, G, P, pb::GROUPED_WAVE_ROWS, nullptr, nullptr);
}

int pb_fista_grouped_route(const int32_t* offsets_host, int G, int P, int N, int K, unsigned flags, int* main_units, int* row_cut) {
  GroupedRoute r{-1, 0, 0, nullptr};
  if (P > 0 && P <= (1 << 25) && N >= 1 && K >= 1 && G >= 0 && pb::grouped_offsets_ok(offsets_host, G, P))
    r = route_grouped(offsets_host, G, P, N, K, flags, true);
  if (main_units) *main_units = r.main_units;
  if (row_cut) *row_cut = r.row_cut;
  return r.code;
}

int pb_fista_solve_grouped(const float* y_dev, int64_t ldy, double* w_dev, int64_t ldw, int P, int N,
                           const double* taps_dev, int64_t ldt, int K, const double* step_dev, int G,
                           const int32_t* offsets_host, const int32_t* offsets_dev, double lbda,
                           const double* lbda_dev, const double* betas_dev, int n_iter, int32_t* n_done_dev,
                           int32_t* work_dev, int64_t work_len, unsigned flags, void* stream) {
  if (P < 0 || N < 1 || K < 1 || n_iter < 0 || G < 0)
    return fail(PB_ERR_INVALID, "pb_fista_solve_grouped: bad size (P=%d N=%d K=%d n_iter=%d G=%d)", P, N, K, n_iter, G);
  if (P > (1 << 25)) return fail(PB_ERR_INVALID, "pb_fista_solve_grouped: more than 2^25 problems per launch");
  if (ldy < N || ldw < N || ldt < K) return fail(PB_ERR_INVALID, "pb_fista_solve_grouped: leading dimension too small");
  if (!pb::grouped_offsets_ok(offsets_host, G, P))
    return fail(PB_ERR_INVALID, "pb_fista_solve_grouped: offsets must run 0 = offsets[0] <= ... <= offsets[G] = P (host memory)");
  if (P == 0) return PB_OK;
  if (!y_dev || !w_dev || !taps_dev || !step_dev || !offsets_dev || !work_dev || (n_iter > 0 && !betas_dev))
    return fail(PB_ERR_INVALID, "pb_fista_solve_grouped: NULL pointer");
  const GroupedWork wl = grouped_work(P, G, K);
  if (work_len < wl.total || (reinterpret_cast<uintptr_t>(work_dev) & 7) != 0)
    return fail(PB_ERR_INVALID, "pb_fista_solve_grouped: work buffer must hold %lld int32 words (pb_fista_grouped_work_len), 8-byte aligned",
                (long long)wl.total);
  // the decision (dispatch.h: route_grouped -- what pb_fista_grouped_route reports)
  const GroupedRoute gr = route_grouped(offsets_host, G, P, N, K, flags, n_done_dev != nullptr);
  if (gr.code < 0) {
    if ((flags & PB_FLAG_GROUPED_SPLIT) && N > MFMA1_NMAX)
      return fail(PB_ERR_INVALID, "pb_fista_solve_grouped: no matrix-pipe form for N=%d K=%d (with PB_FLAG_GROUPED_SPLIT: 311 .. 1 280 scans, K <= %d, n_done_dev given)",
                  N, K, GROUPED_SPLIT_KMAX);
    return fail(PB_ERR_INVALID, "pb_fista_solve_grouped: no matrix-pipe form for N=%d K=%d (129 .. 310 scans, K <= 33, n_done_dev given)", N, K);
  }
  const grouped_launch_fn mf = gr.fn;
  const bool use_mfma = gr.code > 0;
  const bool resolve = !(flags & PB_FLAG_CERT_NO_RESOLVE);
  const hipStream_t user = (hipStream_t)stream;
  int32_t* first = work_dev + wl.first;
  int32_t* table = work_dev + wl.table;
  const int32_t* n_units_dev = first + G;
  double* taps_rows = reinterpret_cast<double*>(work_dev + wl.taps);
  double* step_rows = reinterpret_cast<double*>(work_dev + wl.steps);
  const int units = pb::grouped_table(offsets_host, G, P, pb::GROUPED_WAVE_ROWS, nullptr, nullptr);     // (P > 0: at least one)
  launch_grouped_table(offsets_dev, G, P, pb::GROUPED_WAVE_ROWS, (int)pb::grouped_max_units(P, G, pb::GROUPED_WAVE_ROWS), first, table, user);
  // `main_units` units of the table run on the matrix pipe (whole rounds or passes and, where it pays, the rest), the rows
  // from `row_cut` on -- the first row of the first unit left out -- on the vector forms behind them
  const int main_units = use_mfma ? gr.main_units : units, row_cut = use_mfma ? gr.row_cut : P;
  if (!use_mfma || resolve || row_cut < P)
    hipLaunchKernelGGL(pb::grouped_expand_kernel, dim3((unsigned)((units + 3) / 4)), dim3(256), 0, user, table, n_units_dev, taps_dev,
                       ldt, K, step_dev, taps_rows, step_rows);
  int rc = check_launch("pb_fista_solve_grouped: unit table");
  if (rc != PB_OK) return rc;
  const unsigned vector_flags = flags & ~(PB_FLAG_FORCE_MFMA | PB_FLAG_NO_MFMA | PB_FLAG_GROUPED_SPLIT);
  if (!use_mfma)
    return pb_fista_solve_pp(y_dev, ldy, w_dev, ldw, P, N, taps_rows, K, K, step_rows, lbda, lbda_dev, betas_dev, n_iter, PB_STOP_NONE,
                             0.0, n_done_dev, vector_flags, stream);
  pb::FistaArgs a = fista_args(P, N, K, n_iter, 1, ldy, w_dev, ldw, 0.0, lbda, lbda_dev, betas_dev, PB_STOP_NONE, 0.0, n_done_dev, flags);
  a.y = y_dev; a.taps_pp = taps_dev; a.ldt = ldt; a.step_vec = step_dev; a.step_shared = 0;
  a.perm = table; a.n_dense = n_units_dev; a.grid_slots = main_units;     // (one wave per unit: whole rounds are a multiple of the four waves of a workgroup; the split forms: one workgroup per unit)
  if (mf(a, K, user) != 0) return fail(PB_ERR_INVALID, "pb_fista_solve_grouped: the matrix-pipe kernel rejected its launch");
  rc = check_launch(gr.code == 4 ? "fista_mfma_kernel(grouped)" : gr.code == 5 ? "fista_mfma2_kernel(grouped)" : "fista_mfma4_kernel(grouped)");
  if (rc != PB_OK) return rc;
  // the per-problem vector forms, every row with its parcel's taps: the rows behind the whole rounds, then what the
  // guards handed back (n_done = -1)
  pb::FistaArgs b = fista_args(P, N, K, n_iter, 1, ldy, w_dev, ldw, 0.0, lbda, lbda_dev, betas_dev, PB_STOP_NONE, 0.0, n_done_dev, flags);
  b.y = y_dev; b.taps_pp = taps_rows; b.ldt = K; b.step_vec = step_rows; b.step_shared = 0;
  if (row_cut < P) {
    const Route rr = route_pp(N, K, P - row_cut, false, PB_STOP_NONE, true, 0u);
    if (rr.path != PATH_PIECES && rr.path != PATH_WIDE)
      return fail(PB_ERR_INVALID, "pb_fista_solve_grouped: no vector form for N=%d K=%d", N, K);
    pb::FistaArgs c = b;
    c.p0 = row_cut;
    rc = launch(DeviceTapsForms{rr, "pb_fista_solve_grouped", K, PB_STOP_NONE}, rr.path == PATH_WIDE ? FORM_WIDE : rr.one_form, c, user);
    if (rc != PB_OK) return rc;
  }
  if (!resolve) return rc;
  b.P = row_cut;
  b.only_flagged = 1;
  const Route r = route_pp(N, K, row_cut, false, PB_STOP_NONE, true, 0u);
  const DeviceTapsForms lf{r, "pb_fista_solve_grouped", K, PB_STOP_NONE};
  if (r.fe) return launch(lf, FORM_FAST1, b, user, true);
  if (r.we) return launch(lf, FORM_WIDE, b, user, true);
  return fail(PB_ERR_INVALID, "pb_fista_solve_grouped: no vector form re-solves N=%d K=%d", N, K);
}

// ---- the conditioning guard of the solves whose HRF lives in device memory (opt-in: the _guarded entry points) ------------
// The marks pass (path.h: marks_wave_kernel) classes every row on gamma_2 with the bounds of the partitioned route; the rows
// with mark 2 (and, where the call's route has a matrix-pipe form, mark 1) are listed on the device (guard.h), their warm
// start saved; the main solve is enqueued by the plain entry point itself, over all rows; then the listed rows get their
// warm start back and are solved again in place, mark 1 on the float32 vector form of the route's own re-solves, mark 2 on a
// float64 kernel with per-problem taps.  Everything on the caller's stream, nothing read on the host.
}  // extern "C"
namespace {
void launch_marks(const float* y, int64_t ldy, int P, int N, const double* taps, int64_t ldt, int K, const int32_t* offsets, int G,
                  int32_t* marks, hipStream_t st) {
  const float g64 = (float)PART_GAMMA_F64, gv = (float)part_gamma_matrix_pipe(N, K);
  const dim3 grid((unsigned)((P + 3) / 4)), block(256);
  if (N <= 320)
    hipLaunchKernelGGL((pb::marks_wave_kernel<5>), grid, block, 4 * (64 * 5 + 2 * pb::LMAX_KT) * sizeof(float), st, y, ldy, P, N, taps,
                       ldt, K, offsets, G, g64, gv, marks);
  else if (N <= 640)
    hipLaunchKernelGGL((pb::marks_wave_kernel<10>), grid, block, 4 * (64 * 10 + 2 * pb::LMAX_KT) * sizeof(float), st, y, ldy, P, N, taps,
                       ldt, K, offsets, G, g64, gv, marks);
  else
    hipLaunchKernelGGL((pb::marks_wave_kernel<21>), grid, block, 4 * (64 * 21 + 2 * pb::LMAX_KT) * sizeof(float), st, y, ldy, P, N, taps,
                       ldt, K, offsets, G, g64, gv, marks);
}
static_assert(pb::MARKS_KMAX == pb::LMAX_KT, "one tap limit for the two marks passes");

// the float64 kernel that re-solves the rows with mark 2 (per-problem taps, float32 y): code 1 the one-wave register form,
// 2 four waves, 3 / 4 the same for HRFs of 33 .. 48 taps, 5 the LDS kernel; 0: the shape has none, or the marks pass does
// not carry it (more than 64 taps or 1 344 scans) -- no guard
struct GuardKernel { int code; const ExactEntry* e; };
GuardKernel guard_kernel(int N, int K, int stop_mode) {
  if (N < 1 || N > pb::MARKS_NMAX || K < 1 || K > pb::MARKS_KMAX) return {0, nullptr};
  if (stop_mode != PB_STOP_NONE && stop_mode != PB_STOP_LOOPS) return {0, nullptr};
  static const int forms[4] = {F64_ONE_WAVE, F64_FOUR_WAVES, F64_LONG_HRF, F64_FOUR_WAVES_LONG_HRF};
  for (int i = 0; i < 4; ++i) {
    const ExactEntry* e = pick_f64(forms[i], N, K, stop_mode, F64_WIND);
    if (e) return {i + 1, e};
  }
  return {gen_lds_doubles(N, K, stop_mode, 0) <= LDS_DOUBLES_MAX ? 5 : 0, nullptr};
}

struct GuardCall {
  const char* name;
  int32_t* work;
  pb::GuardLayout gl;
  GuardKernel gk;
  bool want_vec, cold;
  hipStream_t st;
};
int guard_work_check(const char* name, int P, int N, unsigned flags, const int32_t* work_dev, int64_t work_len) {
  const pb::GuardLayout gl = pb::guard_layout(P, N, (flags & PB_FLAG_COLD_START) != 0);
  if (!work_dev || work_len < gl.total || (reinterpret_cast<uintptr_t>(work_dev) & 7) != 0)
    return fail(PB_ERR_INVALID, "%s: guard work buffer must hold %lld int32 words (pb_fista_guard_work_len), 8-byte aligned", name,
                (long long)gl.total);
  return PB_OK;
}
// what pb_fista_solve_pp would refuse once its route is known (checked before the guard's first launch)
int pp_route_check(const char* name, const Route& r, int N, int K, int stop_mode, unsigned flags) {
  if (r.path != PATH_GENERIC) return PB_OK;
  if (flags & PB_FLAG_FORCE_FAST) return fail(PB_ERR_INVALID, "%s: no register-resident kernel for N=%d K=%d", name, N, K);
  if (gen_lds_doubles(N, K, stop_mode, 0) > LDS_DOUBLES_MAX) return fail(PB_ERR_INVALID, "%s: N=%d K=%d exceeds LDS", name, N, K);
  return PB_OK;
}
// a route of pb_fista_solve_pp puts rows on a matrix-pipe form: whole passes of a split form, or a piece of the plan of the
// single-row entry's forms
bool pp_route_has_pipe(const Route& r, int P, unsigned flags) {
  if (r.path == PATH_SPLIT_LONG) return r.base > 0;
  if (r.path != PATH_PIECES || !r.mfma || r.one_form) return false;
  Piece pc[pb::MAX_PIECES];
  const int npc = route_pieces(r, P, (flags & PB_FLAG_ONE_LAUNCH) != 0, true, pc);
  bool pipe = false;
  for (int i = 0; i < npc; ++i) pipe |= pc[i].form == FORM_MFMA || pc[i].form == FORM_MFMA2;
  return pipe;
}
// a call without a guard (no float64 kernel for the shape, too many taps): the header says "no row listed"
int guard_none(const GuardCall& g) {
  if (hipMemsetAsync(g.work, 0, pb::GUARD_HEADER * sizeof(int32_t), g.st) != hipSuccess)
    return fail(PB_ERR_HIP, "%s: clearing the guard header failed", g.name);
  return PB_OK;
}
// before the main solve: marks, lists, the warm start of the listed rows
int guard_before(const GuardCall& g, const float* y, int64_t ldy, double* w, int64_t ldw, int P, int N, const double* taps, int64_t ldt,
                 int K, const int32_t* offsets_dev, int G) {
  launch_marks(y, ldy, P, N, taps, ldt, K, offsets_dev, G, g.work + g.gl.marks, g.st);
  pb::launch_mark_lists(P, g.want_vec ? 1 : 0, g.work, g.gl, g.st);
  if (!g.cold) pb::launch_rows_move(true, P, N, w, ldw, g.work, g.gl, g.st);
  return check_launch(g.name);
}
// after it: the warm start back, then the two lists in place.  `b`: the call's arguments with per-problem (or shared, ldt = 0)
// taps and steps; `lf`, `vec_form`: the float32 vector form of the route's own re-solves
template <class LF>
int guard_after(const GuardCall& g, const pb::FistaArgs& a, const LF& lf, int vec_form) {
  const int P = a.P;
  if (!g.cold) pb::launch_rows_move(false, P, a.N, a.w, a.ldw, g.work, g.gl, g.st);
  int rc = check_launch(g.name);
  if (rc != PB_OK) return rc;
  pb::FistaArgs b = a;
  b.perm_side = 3;
  b.grid_slots = P;
  if (g.want_vec) {
    b.perm = g.work + g.gl.listv;
    b.range = g.work + 2;
    rc = launch(lf, vec_form, b, g.st, true);
    if (rc != PB_OK) return rc;
  }
  b.perm = g.work + g.gl.list64;
  b.range = g.work;
  if (g.gk.e) {
    if (a.step_shared) {                          // (the float64 register kernels read step_vec[p])
      double* steps = reinterpret_cast<double*>(g.work + g.gl.steps);
      pb::launch_steps_fill(a.step_vec, steps, P, g.st);
      b.step_vec = steps;
      b.step_shared = 0;
    }
    if (g.gk.e->fn_pp(b, false, a.stop_mode, g.st) != 0)
      return fail(PB_ERR_INVALID, "%s: float64 kernel rejected the launch (ill-conditioned series)", g.name);
  } else {
    launch_generic(b, a.taps_pp, a.K, 0, false, false, P < 2048 ? P : 2048, g.st);
  }
  return check_launch("float64 kernel (ill-conditioned series)");
}
}  // namespace
extern "C" {

int64_t pb_fista_guard_work_len(int P, int N, unsigned flags) {
  return (P >= 0 && N >= 1) ? pb::guard_layout(P, N, (flags & PB_FLAG_COLD_START) != 0).total : 0;
}

int pb_fista_guard_supported(int N, int K, int stop_mode) { return guard_kernel(N, K, stop_mode).code; }

int pb_fista_pp_has_matrix_pipe(int N, int K, int P, int shared, int stop_mode, unsigned flags) {
  if (P < 1 || N < 1 || K < 1) return 0;
  return pp_route_has_pipe(route_pp(N, K, P, shared != 0, stop_mode, true, flags), P, flags) ? 1 : 0;
}

int pb_conditioning_marks(const float* y_dev, int64_t ldy, int P, int N, const double* taps_dev, int64_t ldt, int K,
                          const int32_t* offsets_dev, int G, int32_t* marks_dev, void* stream) {
  if (P < 0 || N < 1 || N > pb::MARKS_NMAX || K < 1 || K > pb::MARKS_KMAX)
    return fail(PB_ERR_INVALID, "pb_conditioning_marks: bad size (P=%d N=%d K=%d; up to %d scans and %d taps)", P, N, K, pb::MARKS_NMAX,
                pb::MARKS_KMAX);
  if (ldy < N || (ldt != 0 && ldt < K)) return fail(PB_ERR_INVALID, "pb_conditioning_marks: leading dimension too small");
  if (offsets_dev && G < 1) return fail(PB_ERR_INVALID, "pb_conditioning_marks: offsets given for G=%d parcels", G);
  if (P == 0) return PB_OK;
  if (!y_dev || !taps_dev || !marks_dev) return fail(PB_ERR_INVALID, "pb_conditioning_marks: NULL pointer");
  launch_marks(y_dev, ldy, P, N, taps_dev, ldt, K, offsets_dev, G, marks_dev, (hipStream_t)stream);
  return check_launch("pb_conditioning_marks");
}

int pb_fista_solve_pp_guarded(const float* y_dev, int64_t ldy, double* w_dev, int64_t ldw, int P, int N,
                              const double* taps_dev, int64_t ldt, int K, const double* step_dev,
                              double lbda, const double* lbda_dev, const double* betas_dev, int n_iter,
                              int stop_mode, double tol, int32_t* n_done_dev, int32_t* work_dev, int64_t work_len,
                              unsigned flags, void* stream) {
  static const char* const name = "pb_fista_solve_pp_guarded";
  if (P < 0 || N < 1 || K < 1 || n_iter < 0)
    return fail(PB_ERR_INVALID, "%s: bad size (P=%d N=%d K=%d n_iter=%d)", name, P, N, K, n_iter);
  if (P > (1 << 25)) return fail(PB_ERR_INVALID, "%s: more than 2^25 problems per launch", name);
  if (ldy < N || ldw < N || (ldt != 0 && ldt < K)) return fail(PB_ERR_INVALID, "%s: leading dimension too small", name);
  if (P == 0) return PB_OK;
  if (!y_dev || !w_dev || !taps_dev || !step_dev || (n_iter > 0 && !betas_dev)) return fail(PB_ERR_INVALID, "%s: NULL pointer", name);
  if (!n_done_dev) return fail(PB_ERR_INVALID, "%s: n_done_dev is required", name);
  if (stop_mode != PB_STOP_NONE && stop_mode != PB_STOP_LOOPS)
    return fail(PB_ERR_INVALID, "%s: stop_mode must be PB_STOP_NONE or PB_STOP_LOOPS", name);
  int rc = guard_work_check(name, P, N, flags, work_dev, work_len);
  if (rc != PB_OK) return rc;
  const Route r = route_pp(N, K, P, ldt == 0, stop_mode, true, flags);
  rc = pp_route_check(name, r, N, K, stop_mode, flags);
  if (rc != PB_OK) return rc;
  GuardCall g{name, work_dev, pb::guard_layout(P, N, (flags & PB_FLAG_COLD_START) != 0), guard_kernel(N, K, stop_mode), false,
              (flags & PB_FLAG_COLD_START) != 0, (hipStream_t)stream};
  if (!g.gk.code) {
    rc = guard_none(g);
    return rc != PB_OK ? rc : pb_fista_solve_pp(y_dev, ldy, w_dev, ldw, P, N, taps_dev, ldt, K, step_dev, lbda, lbda_dev, betas_dev,
                                                n_iter, stop_mode, tol, n_done_dev, flags, stream);
  }
  // the vector list is needed where the route puts rows on the matrix pipe
  g.want_vec = pp_route_has_pipe(r, P, flags);
  const int vec_form = (r.path == PATH_SPLIT_LONG && r.backup_wide) ? FORM_WIDE : FORM_FAST1;
  rc = guard_before(g, y_dev, ldy, w_dev, ldw, P, N, taps_dev, ldt, K, nullptr, 0);
  if (rc != PB_OK) return rc;
  rc = pb_fista_solve_pp(y_dev, ldy, w_dev, ldw, P, N, taps_dev, ldt, K, step_dev, lbda, lbda_dev, betas_dev, n_iter, stop_mode, tol,
                         n_done_dev, flags, stream);
  if (rc != PB_OK) return rc;
  pb::FistaArgs a = fista_args(P, N, K, n_iter, 1, ldy, w_dev, ldw, 0.0, lbda, lbda_dev, betas_dev, stop_mode, tol, n_done_dev, flags);
  a.y = y_dev; a.taps_pp = taps_dev; a.ldt = ldt; a.step_vec = step_dev; a.step_shared = (ldt == 0);
  return guard_after(g, a, DeviceTapsForms{r, name, K, stop_mode}, vec_form);
}

int pb_fista_solve_grouped_guarded(const float* y_dev, int64_t ldy, double* w_dev, int64_t ldw, int P, int N,
                                   const double* taps_dev, int64_t ldt, int K, const double* step_dev, int G,
                                   const int32_t* offsets_host, const int32_t* offsets_dev, double lbda,
                                   const double* lbda_dev, const double* betas_dev, int n_iter, int32_t* n_done_dev,
                                   int32_t* work_dev, int64_t work_len, int32_t* guard_work_dev, int64_t guard_work_len,
                                   unsigned flags, void* stream) {
  static const char* const name = "pb_fista_solve_grouped_guarded";
  if (P < 0 || N < 1 || K < 1 || n_iter < 0 || G < 0)
    return fail(PB_ERR_INVALID, "%s: bad size (P=%d N=%d K=%d n_iter=%d G=%d)", name, P, N, K, n_iter, G);
  if (P > (1 << 25)) return fail(PB_ERR_INVALID, "%s: more than 2^25 problems per launch", name);
  if (ldy < N || ldw < N || ldt < K) return fail(PB_ERR_INVALID, "%s: leading dimension too small", name);
  if (!pb::grouped_offsets_ok(offsets_host, G, P))
    return fail(PB_ERR_INVALID, "%s: offsets must run 0 = offsets[0] <= ... <= offsets[G] = P (host memory)", name);
  if (P == 0) return PB_OK;
  if (!y_dev || !w_dev || !taps_dev || !step_dev || !offsets_dev || !work_dev || (n_iter > 0 && !betas_dev))
    return fail(PB_ERR_INVALID, "%s: NULL pointer", name);
  if (!n_done_dev) return fail(PB_ERR_INVALID, "%s: n_done_dev is required", name);
  const GroupedWork wl = grouped_work(P, G, K);
  if (work_len < wl.total || (reinterpret_cast<uintptr_t>(work_dev) & 7) != 0)
    return fail(PB_ERR_INVALID, "%s: work buffer must hold %lld int32 words (pb_fista_grouped_work_len), 8-byte aligned", name,
                (long long)wl.total);
  int rc = guard_work_check(name, P, N, flags, guard_work_dev, guard_work_len);
  if (rc != PB_OK) return rc;
  const GroupedRoute gr = route_grouped(offsets_host, G, P, N, K, flags, true);
  if (gr.code < 0) return fail(PB_ERR_INVALID, "%s: no matrix-pipe form for N=%d K=%d under these flags", name, N, K);
  const unsigned vector_flags = flags & ~(PB_FLAG_FORCE_MFMA | PB_FLAG_NO_MFMA | PB_FLAG_GROUPED_SPLIT);
  if (gr.code == 0) {
    rc = pp_route_check(name, route_pp(N, K, P, false, PB_STOP_NONE, true, vector_flags), N, K, PB_STOP_NONE, vector_flags);
    if (rc != PB_OK) return rc;
  }
  const hipStream_t user = (hipStream_t)stream;
  GuardCall g{name, guard_work_dev, pb::guard_layout(P, N, (flags & PB_FLAG_COLD_START) != 0), guard_kernel(N, K, PB_STOP_NONE),
              gr.code > 0, (flags & PB_FLAG_COLD_START) != 0, user};
  // the float32 vector form of the plain call's re-solve of handed-back rows
  const Route rv = route_pp(N, K, gr.code > 0 ? gr.row_cut : P, false, PB_STOP_NONE, true, 0u);
  if (g.gk.code && g.want_vec && !rv.fe && !rv.we) g.gk.code = 0;
  if (!g.gk.code) {
    rc = guard_none(g);
    return rc != PB_OK ? rc : pb_fista_solve_grouped(y_dev, ldy, w_dev, ldw, P, N, taps_dev, ldt, K, step_dev, G, offsets_host,
                                                     offsets_dev, lbda, lbda_dev, betas_dev, n_iter, n_done_dev, work_dev, work_len,
                                                     flags, stream);
  }
  rc = guard_before(g, y_dev, ldy, w_dev, ldw, P, N, taps_dev, ldt, K, offsets_dev, G);
  if (rc != PB_OK) return rc;
  rc = pb_fista_solve_grouped(y_dev, ldy, w_dev, ldw, P, N, taps_dev, ldt, K, step_dev, G, offsets_host, offsets_dev, lbda, lbda_dev,
                              betas_dev, n_iter, n_done_dev, work_dev, work_len, flags, stream);
  if (rc != PB_OK) return rc;
  // every row's copy of its parcel's taps and step in the grouped workspace: written by the plain call unless its main form
  // carried every row and the caller asked for no re-solve
  double* taps_rows = reinterpret_cast<double*>(work_dev + wl.taps);
  double* step_rows = reinterpret_cast<double*>(work_dev + wl.steps);
  if (gr.code > 0 && (flags & PB_FLAG_CERT_NO_RESOLVE) && gr.row_cut >= P) {
    const int units = pb::grouped_table(offsets_host, G, P, pb::GROUPED_WAVE_ROWS, nullptr, nullptr);
    hipLaunchKernelGGL(pb::grouped_expand_kernel, dim3((unsigned)((units + 3) / 4)), dim3(256), 0, user, work_dev + wl.table,
                       work_dev + wl.first + G, taps_dev, ldt, K, step_dev, taps_rows, step_rows);
  }
  pb::FistaArgs a = fista_args(P, N, K, n_iter, 1, ldy, w_dev, ldw, 0.0, lbda, lbda_dev, betas_dev, PB_STOP_NONE, 0.0, n_done_dev, flags);
  a.y = y_dev; a.taps_pp = taps_rows; a.ldt = K; a.step_vec = step_rows; a.step_shared = 0;
  return guard_after(g, a, DeviceTapsForms{rv, name, K, PB_STOP_NONE}, rv.fe ? FORM_FAST1 : FORM_WIDE);
}

int64_t pb_hrf_normal_eq_w_grouped_work_len(int V, int G, int K) {
  return (V >= 0 && G >= 0 && K >= 1) ? ne_grouped_work(V, G, K).total : 0;
}

int pb_hrf_normal_eq_w_grouped(const double* w_dev, int64_t ldw, const float* y_dev, int64_t ldy, int V,
                               int N, int K, int G, const int32_t* offsets_host, const int32_t* offsets_dev,
                               double* work_dev, int64_t work_len, double* out_dev, int64_t ldo, void* stream) {
  if (V < 0 || N < 1 || K < 1 || K > 127 || G < 0 || ldw < N || ldy < N)
    return fail(PB_ERR_INVALID, "pb_hrf_normal_eq_w_grouped: bad size (V=%d N=%d K=%d G=%d)", V, N, K, G);
  const int ne = pb::ne_len(K) + 1;
  if (ldo < ne) return fail(PB_ERR_INVALID, "pb_hrf_normal_eq_w_grouped: ldo < %d", ne);
  if (!pb::grouped_offsets_ok(offsets_host, G, V))
    return fail(PB_ERR_INVALID, "pb_hrf_normal_eq_w_grouped: offsets must run 0 = offsets[0] <= ... <= offsets[G] = V (host memory)");
  if (G == 0) return PB_OK;
  const bool wave_form = ne_wave_form(N, K);
  const int64_t nd = wave_form ? (int64_t)pb::ne_wave_lds_doubles(N, K) : (int64_t)pb::ne_sum_lds_doubles(N, K);
  if (nd > LDS_DOUBLES_MAX) return fail(PB_ERR_INVALID, "pb_hrf_normal_eq_w_grouped: N=%d K=%d exceeds LDS", N, K);
  if (!out_dev || !offsets_dev || !work_dev || (V > 0 && (!w_dev || !y_dev)))
    return fail(PB_ERR_INVALID, "pb_hrf_normal_eq_w_grouped: NULL pointer");
  const NeGroupedWork wl = ne_grouped_work(V, G, K);
  if (work_len < wl.total)
    return fail(PB_ERR_INVALID, "pb_hrf_normal_eq_w_grouped: work buffer must hold %lld doubles (pb_hrf_normal_eq_w_grouped_work_len)",
                (long long)wl.total);
  const hipStream_t user = (hipStream_t)stream;
  const int per = ne_grouped_rows(V);
  int32_t* first = reinterpret_cast<int32_t*>(work_dev);
  int32_t* table = first + (((int64_t)G + 2) & ~(int64_t)1);
  double* part = work_dev + wl.part;
  const int units = pb::grouped_table(offsets_host, G, V, per, nullptr, nullptr);
  launch_grouped_table(offsets_dev, G, V, per, (int)wl.max_units, first, table, user);
  if (units > 0) {
    const size_t lds = (size_t)nd * sizeof(double);
    if (wave_form && K * K <= 64 * 12 && N <= 64 * 5)
      hipLaunchKernelGGL((pb::normal_eq_wave_grouped_kernel<float, 12, 5>), dim3(units), dim3(pb::NE_THREADS), lds, user, w_dev, ldw,
                         y_dev, ldy, table, first + G, N, K, part);
    else if (wave_form)
      hipLaunchKernelGGL((pb::normal_eq_wave_grouped_kernel<float>), dim3(units), dim3(pb::NE_THREADS), lds, user, w_dev, ldw, y_dev,
                         ldy, table, first + G, N, K, part);
    else
      hipLaunchKernelGGL((pb::normal_eq_sum_grouped_kernel<float>), dim3(units), dim3(pb::NE_THREADS), lds, user, w_dev, ldw, y_dev,
                         ldy, table, first + G, N, K, part);
  }
  // second stage: entries per workgroup from the largest parcel (few units: wide workgroups; many: a tree per entry),
  // raised until the grid stays below 2^16 workgroups
  int max_units = 0;
  for (int g = 0; g < G; ++g) {
    const int n = (offsets_host[g + 1] - offsets_host[g] + per - 1) / per;
    max_units = n > max_units ? n : max_units;
  }
  int e_log2 = max_units <= 4 ? 8 : (max_units <= 16 ? 6 : (max_units <= 64 ? 4 : (max_units <= 256 ? 2 : 0)));
  while (e_log2 < 8 && (int64_t)G * ((ne + (1 << e_log2) - 1) >> e_log2) > 65536) ++e_log2;
  const int64_t chunks = (ne + (1 << e_log2) - 1) >> e_log2;
  hipLaunchKernelGGL(pb::normal_eq_reduce_grouped_kernel, dim3((unsigned)(G * chunks)), dim3(pb::NE_THREADS), 0, user, part, first, G,
                     ne, e_log2, out_dev, ldo);
  return check_launch("pb_hrf_normal_eq_w_grouped");
}

int64_t pb_fista_path_work_len(int P) { return P >= 0 ? work_layout(P, P).total : 0; }     // (enough for any y_rep)

int pb_fista_solve_path(const float* y_dev, int64_t ldy, int y_rep, double* w_dev, int64_t ldw, int P, int N,
                        const double* taps_host, const double* taps_dev, int K, double step,
                        const double* lbda_dev, const double* lmax_dev, double dense_ratio,
                        const double* betas_dev, int n_iter, int32_t* n_done_dev, int32_t* work_dev,
                        int64_t work_len, unsigned flags, void* stream) {
  // (pb_fista_solve_ex with per-problem lambdas, the caller's lambda_max and workspace)
  if (P > 0 && (!lbda_dev || !n_done_dev))
    return fail(PB_ERR_INVALID, "pb_fista_solve_path: NULL pointer (per-problem lambdas and n_done are required)");
  return solve_impl(y_dev, ldy, y_rep, w_dev, ldw, P, N, taps_host, taps_dev, K, step, 0.0, lbda_dev, betas_dev, n_iter,
                    nullptr, 0, PB_STOP_NONE, 0.0, 6, n_done_dev, flags, stream, lmax_dev, dense_ratio, work_dev, work_len);
}

}  // extern "C"
