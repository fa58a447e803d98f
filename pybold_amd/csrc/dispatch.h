// The dispatch of the FISTA entry points (private to capi.hip, included once: internal linkage throughout): the tables of
// kernel instantiations, the pickers of an entry for a shape, the thresholds and flag masks, and the route of a call --
// `route` for the calls with the taps on the host, `route_pp` for pb_fista_solve_pp -- with what the queries report of
// it.  Nothing here launches a kernel: capi.hip validates, runs a route (its executors) and holds the C entry points.
#pragma once
#include "../../include/pybold_hip.h"
#include "fista_fast.h"
#include "launch_fast.h"
#include "fista_pair.h"
#include "fista_pair_ffa.h"
#include "fista_exact.h"
#include "fista_exact_split.h"
#include "fista_auto.h"
#include "fista_auto_split.h"
#include "fista_exact_pp.h"
#include "fista_exact_long.h"
#include "fista_exact_split_long.h"
#include "fista_mfma.h"
#include "fista_mfma2.h"
#include "fista_mfma4.h"
#include "path.h"

namespace {

// ---- register-resident specialisations --------------------------------------
typedef int (*fast_launch_fn)(const pb::FistaArgs&, const double* taps, int K, bool with_j,
                              int stop, hipStream_t);
typedef int (*fast_launch_pp_fn)(const pb::FistaArgs&, int stop, hipStream_t);
// the pair form and the three matrix-pipe forms
typedef int (*launch_fn)(const pb::FistaArgs&, const double* taps, int K, bool with_j, hipStream_t);
typedef int (*pair_cert_fn)(const pb::FistaArgs&, const double* taps, int K, hipStream_t);
typedef int (*pair_split_fn)(const pb::FistaArgs&, const double* taps, int K, bool with_j, bool cert, hipStream_t);

struct FastEntry {
  int S, KT;
  fast_launch_fn fn;
  fast_launch_pp_fn fn_pp;
  launch_fn fn_pair;          // two-problems-per-row kernel (S <= 20, KT <= 32 only), else nullptr
  launch_fn fn_pair_ffa;      // the same with 2-parallel fast FIRs (fista_pair_ffa.h)
  int (*fn_pair_dev)(const pb::FistaArgs&, hipStream_t);   // ... reading ONE shared HRF from device memory
  pair_cert_fn fn_pair_cert;  // ... carrying the window rule (wind = 6) as a no-fire certificate
  pair_split_fn fn_pair_split; // ... ONE series of 16 S < N <= 32 S scans per row (its halves in the two slots)
};

}  // namespace

// instantiated in fast_inst.hip, one translation unit per table entry
namespace pb {
#define PB_FAST(S, KT)                                                                              \
  extern template int launch_fast<S, KT>(const FistaArgs&, const double*, int, bool, int, hipStream_t); \
  extern template int launch_fast_pp<S, KT>(const FistaArgs&, int, hipStream_t);            \
  extern template int launch_pair<S, KT>(const FistaArgs&, const double*, int, bool, hipStream_t); \
  extern template int launch_pair_ffa<S, KT>(const FistaArgs&, const double*, int, bool, hipStream_t); \
  extern template int launch_pair_ffa_dev<S, KT>(const FistaArgs&, hipStream_t);                  \
  extern template int launch_pair_ffa_cert<S, KT>(const FistaArgs&, const double*, int, hipStream_t); \
  extern template int launch_pair_ffa_split<S, KT>(const FistaArgs&, const double*, int, bool, bool, hipStream_t);
#include "fast_table.inc"
#undef PB_FAST
}  // namespace pb

namespace pb {
#define PB_MFMA(NB) extern template int launch_mfma<NB>(const FistaArgs&, const double*, int, bool, hipStream_t);
PB_MFMA(5) PB_MFMA(6) PB_MFMA(7) PB_MFMA(8) PB_MFMA(9) PB_MFMA(10)
#undef PB_MFMA
// (fista_mfma_sparse.h: the plain solve with K <= 32 on the 2:4-sparse near tiles, every other call on launch_mfma<NB>)
#define PB_MFMA(NB) extern template int launch_mfma_st<NB>(const FistaArgs&, const double*, int, bool, hipStream_t);
PB_MFMA(5) PB_MFMA(6) PB_MFMA(7) PB_MFMA(8) PB_MFMA(9) PB_MFMA(10)
#undef PB_MFMA
// (fista_mfma_grouped.h: the same two kernels with one HRF per parcel, pb_fista_solve_grouped)
#define PB_MFMA(NB) extern template int launch_mfma_grouped<NB>(const FistaArgs&, int, hipStream_t);
PB_MFMA(5) PB_MFMA(6) PB_MFMA(7) PB_MFMA(8) PB_MFMA(9) PB_MFMA(10)
#undef PB_MFMA
}
namespace pb {
#define PB_MFMA2(A, B) extern template int launch_mfma2<A, B>(const FistaArgs&, const double*, int, bool, hipStream_t);
PB_MFMA2(2, 3) PB_MFMA2(3, 3) PB_MFMA2(3, 4) PB_MFMA2(4, 4) PB_MFMA2(4, 5) PB_MFMA2(5, 5) PB_MFMA2(5, 6) PB_MFMA2(6, 6)
PB_MFMA2(6, 7) PB_MFMA2(7, 7) PB_MFMA2(7, 8) PB_MFMA2(8, 8) PB_MFMA2(8, 9) PB_MFMA2(9, 9) PB_MFMA2(9, 10) PB_MFMA2(10, 10)
#undef PB_MFMA2
#define PB_MFMA4(A) extern template int launch_mfma4<A>(const FistaArgs&, const double*, int, bool, hipStream_t);
PB_MFMA4(6) PB_MFMA4(7) PB_MFMA4(8) PB_MFMA4(9) PB_MFMA4(10)
#undef PB_MFMA4
// (fista_mfma_split_grouped.h: the two split kernels with one HRF per parcel, pb_fista_solve_grouped with PB_FLAG_GROUPED_SPLIT)
#define PB_MFMA2(A, B) extern template int launch_mfma2_grouped<A, B>(const FistaArgs&, int, hipStream_t);
PB_MFMA2(5, 5) PB_MFMA2(5, 6) PB_MFMA2(6, 6) PB_MFMA2(6, 7) PB_MFMA2(7, 7) PB_MFMA2(7, 8) PB_MFMA2(8, 8) PB_MFMA2(8, 9) PB_MFMA2(9, 9)
PB_MFMA2(9, 10) PB_MFMA2(10, 10)
#undef PB_MFMA2
#define PB_MFMA4(A) extern template int launch_mfma4_grouped<A>(const FistaArgs&, int, hipStream_t);
PB_MFMA4(6) PB_MFMA4(7) PB_MFMA4(8) PB_MFMA4(9) PB_MFMA4(10)
#undef PB_MFMA4
}
namespace {
// the matrix-pipe form with one series split over the two waves of a workgroup (fista_mfma2.h): nb = ceil(N / 32)
// blocks of 32 samples (it keeps the carry tile: its waves are bound by the vector work of the exchange, not by
// their matrix instructions -- the sum-slot form of fista_mfma.h measured 4 % slower there), 5 <= nb <= 20
// (129 .. 640 scans), floor(nb / 2) of them in the left wave; K <= 33; plain solves, the cost
// trace and the window rule (wind = 6) as a no-fire certificate; the shared-HRF z-step plain only
// (34 <= K <= 65: three near tiles -- series of 225+ scans (four blocks per wave; the one-wave form carries shorter ones, and
// everything up to 310 scans but the certificate), plain solves, the cost trace, the certificate and the _loops_deconv rule;
// `two_tiles_only`: K <= 33)
launch_fn pick_mfma2(int N, int K, bool two_tiles_only) {
  static const launch_fn tab[] = {
      &pb::launch_mfma2<2, 3>, &pb::launch_mfma2<3, 3>, &pb::launch_mfma2<3, 4>, &pb::launch_mfma2<4, 4>,
      &pb::launch_mfma2<4, 5>, &pb::launch_mfma2<5, 5>, &pb::launch_mfma2<5, 6>, &pb::launch_mfma2<6, 6>,
      &pb::launch_mfma2<6, 7>, &pb::launch_mfma2<7, 7>, &pb::launch_mfma2<7, 8>, &pb::launch_mfma2<8, 8>,
      &pb::launch_mfma2<8, 9>, &pb::launch_mfma2<9, 9>, &pb::launch_mfma2<9, 10>, &pb::launch_mfma2<10, 10>};
  const int nb = (N + 31) / 32;
  if (K < 1 || K > 65 || nb < 5 || nb > 20) return nullptr;
  if (K > 33 && (two_tiles_only || N <= 224)) return nullptr;   // (three near tiles: four blocks at least per wave)
  return tab[nb - 5];
}
// the same with one series split over the FOUR waves of a workgroup (fista_mfma4.h): 641 .. 1 280 scans, A = ceil(N / 128)
// blocks per wave (6 .. 10); K <= 33 with two near tiles: the call shapes of the two-wave form; 34 <= K <= 65 with three: plain
// solves, the cost trace, the certificate and the _loops_deconv rule (`two_tiles_only`: K <= 33)
launch_fn pick_mfma4(int N, int K, bool two_tiles_only) {
  static const launch_fn tab[] = {&pb::launch_mfma4<6>, &pb::launch_mfma4<7>, &pb::launch_mfma4<8>, &pb::launch_mfma4<9>,
                                  &pb::launch_mfma4<10>};
  if (K < 1 || K > 65 || (K > 33 && two_tiles_only) || N <= 640 || N > 1280) return nullptr;
  return tab[(N + 127) / 128 - 6];
}
// the matrix-pipe form (fista_mfma.h): NB = ceil(N / 31) blocks of 31 samples + one sum slot, 129 <= N <= 310; K <= 33
// with two near tiles (every variant), 34 <= K <= 64 with three (plain solves and the cost trace only: `stop_rule` = the
// window-rule certificate or the _loops_deconv rule rides the kernel)
constexpr int MFMA_K2 = 33, MFMA_K3 = 64;
constexpr int MFMA1_NMAX = 10 * pb::MFMA_SPAN;   // longer series (up to 640 scans) run on the split form (fista_mfma2.h)
// `dense_tiles` (PB_FLAG_MFMA_DENSE_TILES): the plain solve with K <= 32 keeps its two dense near tiles too
launch_fn pick_mfma(int N, int K, bool stop_rule, bool dense_tiles = false) {
  static const launch_fn tab[] = {&pb::launch_mfma<5>, &pb::launch_mfma<6>, &pb::launch_mfma<7>,
                                  &pb::launch_mfma<8>, &pb::launch_mfma<9>, &pb::launch_mfma<10>};
  static const launch_fn tab_st[] = {&pb::launch_mfma_st<5>, &pb::launch_mfma_st<6>, &pb::launch_mfma_st<7>,
                                     &pb::launch_mfma_st<8>, &pb::launch_mfma_st<9>, &pb::launch_mfma_st<10>};
  const int nb = (N + pb::MFMA_SPAN - 1) / pb::MFMA_SPAN;
  if (K < 1 || K > MFMA_K3 || (K > MFMA_K2 && stop_rule) || N <= 128 || nb > 10) return nullptr;   // (129 .. 310 scans: 5 .. 10 blocks)
  return (dense_tiles ? tab : tab_st)[nb - 5];
}
// the grouped z-step (one HRF per parcel): 129 .. 310 scans, K <= 33 (two near tiles), plain solves
typedef int (*grouped_launch_fn)(const pb::FistaArgs&, int K, hipStream_t);
grouped_launch_fn pick_mfma_grouped(int N, int K) {
  static const grouped_launch_fn tab[] = {&pb::launch_mfma_grouped<5>, &pb::launch_mfma_grouped<6>, &pb::launch_mfma_grouped<7>,
                                          &pb::launch_mfma_grouped<8>, &pb::launch_mfma_grouped<9>, &pb::launch_mfma_grouped<10>};
  const int nb = (N + pb::MFMA_SPAN - 1) / pb::MFMA_SPAN;
  if (K < 1 || K > MFMA_K2 || N <= 128 || nb > 10) return nullptr;
  return tab[nb - 5];
}
}  // namespace
namespace pb {
#define PB_WIDE(S, KT)                                                                            \
  extern template int launch_wide<S, KT>(const FistaArgs&, const double*, int, bool, int, hipStream_t); \
  extern template int launch_wide_pp<S, KT>(const FistaArgs&, int, hipStream_t);
#include "wide_table.inc"
#undef PB_WIDE
}  // namespace pb
namespace {

typedef int (*wide_launch_fn)(const pb::FistaArgs&, const double* taps, int K, bool with_j, int stop,
                              hipStream_t);
struct WideEntry {
  int S, KT;
  wide_launch_fn fn;
  fast_launch_pp_fn fn_pp;
};
#define PB_WIDE(S, KT) {S, KT, &pb::launch_wide<S, KT>, &pb::launch_wide_pp<S, KT>},
const WideEntry kWide[] = {
#include "wide_table.inc"
};
#undef PB_WIDE

// cheapest entry of a table (by S * KT) that holds N scans at `per_lane` scans per unit of S, and K taps
template <class Entry>
const Entry* pick_cheapest(const Entry* tab, size_t n, int N, int K, int per_lane) {
  const Entry* best = nullptr;
  const int s_need = (N + per_lane - 1) / per_lane;
  for (const Entry* e = tab; e != tab + n; ++e) {
    if (e->S < s_need || e->KT < K) continue;
    if (!best || (int64_t)e->S * e->KT < (int64_t)best->S * best->KT) best = e;
  }
  return best;
}
template <class Entry, size_t n>
const Entry* pick_cheapest(const Entry (&tab)[n], int N, int K, int per_lane) { return pick_cheapest(tab, n, N, K, per_lane); }
const WideEntry* pick_wide(int N, int K) { return pick_cheapest(kWide, N, K, 64); }

// window lengths the register-resident forms carry (increment ring of wind - 2 slots in LDS)
inline bool ring_wind(int wind) { return wind == 4 || wind == 6 || wind == 8; }
// an entry of S samples per lane carries the call's stop rule: the window rule needs its increment ring (S <= 20)
inline bool ring_fits(int S, int stop_mode, int wind) { return stop_mode != PB_STOP_WINDOW || (ring_wind(wind) && S <= 20); }

// ---- the float64 register-resident family (fista_exact*.h, fista_auto*.h) ------------------------------------------------
// Four forms (F64Form), each with four kinds of launch on the same (S, KT): the solve and the device-resident lambda search,
// with the taps on the host or with one HRF and one step per problem in device memory ("pp").  A form is one table of
// entries (its .inc file) and one descriptor (kF64); pick_f64 is the only picker.  Only the one-wave form, and behind it the
// four-wave form for calls with the taps on the host, is ever chosen by the library (pick_f64_default): every other route to
// a form is OPT-IN, by a flag (PB_FLAG_LONG_HRF, PB_FLAG_PP_SPLIT) or by the name of the entry point.
typedef int (*exact_launch_fn)(const pb::FistaArgs&, const double* taps, int K, bool with_j, int stop, hipStream_t);
typedef int (*auto_launch_fn)(const pb::AutoArgs&, const double* taps, int K, bool early_stopping, hipStream_t);
typedef int (*exact_pp_launch_fn)(const pb::FistaArgs&, bool with_j, int stop, hipStream_t);
typedef int (*auto_pp_launch_fn)(const pb::AutoArgsPP&, bool early_stopping, hipStream_t);
struct ExactEntry {
  int S, KT;
  exact_launch_fn fn;
  auto_launch_fn fn_auto;
  exact_pp_launch_fn fn_pp;
  auto_pp_launch_fn fn_auto_pp;
};
}  // namespace
// the four launches of a pair (S, KT) of a form, instantiated in one translation unit each (Makefile: EXACTFAMILY)
#define PB_F64_EXTERN(SOLVE, SEARCH, S, KT)                                                           \
  extern template int SOLVE<S, KT>(const FistaArgs&, const double*, int, bool, int, hipStream_t);    \
  extern template int SEARCH<S, KT>(const AutoArgs&, const double*, int, bool, hipStream_t);         \
  extern template int SOLVE##_pp<S, KT>(const FistaArgs&, bool, int, hipStream_t);                   \
  extern template int SEARCH##_pp<S, KT>(const AutoArgsPP&, bool, hipStream_t);
#define PB_F64_ENTRY(SOLVE, SEARCH, S, KT) {S, KT, &pb::SOLVE<S, KT>, &pb::SEARCH<S, KT>, &pb::SOLVE##_pp<S, KT>, &pb::SEARCH##_pp<S, KT>},
namespace pb {
#define PB_EXACT(S, KT) PB_F64_EXTERN(launch_exact, launch_auto, S, KT)
#include "exact_table.inc"
#undef PB_EXACT
#define PB_EXACT_SPLIT(S, KT) PB_F64_EXTERN(launch_exact_split, launch_auto_split, S, KT)
#include "exact_split_table.inc"
#undef PB_EXACT_SPLIT
#define PB_EXACT_LONG(S, KT) PB_F64_EXTERN(launch_exact_long, launch_auto_long, S, KT)
#include "exact_long_table.inc"
#undef PB_EXACT_LONG
#define PB_EXACT_SPLIT_LONG(S, KT) PB_F64_EXTERN(launch_exact_split_long, launch_auto_split_long, S, KT)
#include "exact_split_long_table.inc"
#undef PB_EXACT_SPLIT_LONG
}  // namespace pb
namespace {
// one problem per wave (fista_exact.h, fista_auto.h, fista_exact_pp.h)
#define PB_EXACT(S, KT) PB_F64_ENTRY(launch_exact, launch_auto, S, KT)
const ExactEntry kExact[] = {
#include "exact_table.inc"
};
#undef PB_EXACT
// one problem over the four waves of a workgroup, S samples per lane of each wave (fista_exact_split.h, fista_auto_split.h,
// fista_exact_split_pp.h)
#define PB_EXACT_SPLIT(S, KT) PB_F64_ENTRY(launch_exact_split, launch_auto_split, S, KT)
const ExactEntry kExactSplit[] = {
#include "exact_split_table.inc"
};
#undef PB_EXACT_SPLIT
// HRFs of up to 48 taps, the taps in one VGPR pair of the wave (fista_exact_long.h)
#define PB_EXACT_LONG(S, KT) PB_F64_ENTRY(launch_exact_long, launch_auto_long, S, KT)
const ExactEntry kExactLong[] = {
#include "exact_long_table.inc"
};
#undef PB_EXACT_LONG
// ... and the same holder over the four waves of a workgroup (fista_exact_split_long.h)
#define PB_EXACT_SPLIT_LONG(S, KT) PB_F64_ENTRY(launch_exact_split_long, launch_auto_split_long, S, KT)
const ExactEntry kExactSplitLong[] = {
#include "exact_split_long_table.inc"
};
#undef PB_EXACT_SPLIT_LONG
#undef PB_F64_EXTERN
#undef PB_F64_ENTRY

enum F64Form { F64_ONE_WAVE, F64_FOUR_WAVES, F64_LONG_HRF, F64_FOUR_WAVES_LONG_HRF, F64_FORMS };
struct F64FormDesc {
  int n_min, n_max;               // scans
  int k_max;                      // taps
  int per_lane;                   // scans per unit of S: the lanes of a wave, or of the four waves of a workgroup
  const ExactEntry* tab;
  size_t n_tab;
  // the search's outer iterations per launch when the caller leaves the choice to the library (capi.hip: auto_outer_chunk):
  // inner iterations per resident unit and launch, and the units (waves or workgroups) the machine holds at once
  int auto_launch_iters, auto_resident;
  const char* kernels;            // what check_launch is told: fista_exact<kernels>[_pp]_kernel, auto_lbda<kernels>[_pp]_kernel
  const char* label;              // how a message names the form ("%d": k_max) ...
  const char* noun;               // ... and what it calls it
  const char* taps_over;          // ... and how a solve words K > k_max
};
template <size_t n>
constexpr F64FormDesc f64_form(int n_min, int n_max, int k_max, int per_lane, const ExactEntry (&tab)[n], int launch_iters,
                               int resident, const char* kernels, const char* label, const char* noun, const char* taps_over) {
  return F64FormDesc{n_min, n_max, k_max, per_lane, tab, n, launch_iters, resident, kernels, label, noun, taps_over};
}
const F64FormDesc kF64[F64_FORMS] = {
    // one wave: about 65536 inner iterations per wave slot and launch -- 65536 / nb_sub_iter outer iterations for a batch the
    // machine holds at once (2048 waves: 256 compute units, four SIMDs, two waves of this kernel each), fewer in proportion
    // for a larger one, whose launch runs its waves in rounds
    f64_form(1, 640, 32, 64, kExact, 65536, 2048, "", "one-wave", "form", "exceeds %d taps"),
    // four waves (641 .. 1 280 scans): the register report of the search allows two waves per SIMD, i.e. two workgroups per
    // compute unit, 512 resident at once on 256 compute units; an inner iteration of a workgroup takes about twice that of a
    // wave of the one-wave kernel (3.4 us against 1.5 us alone), so half the budget per slot and launch keeps the longest
    // dispatch under 0.25 s (measured 0.14 s at most: profiles/auto_lbda_split.txt)
    f64_form(641, 1280, 32, 64 * pb::SPLIT_WAVES, kExactSplit, 32768, 256 * 2, "_split", "four-wave", "form",
             "exceeds %d taps"),
    // one wave, up to 48 taps: the register reports allow the residency of the one-wave search, but a pass carries 48 taps
    // for 32 (1.5x the multiply-adds, and two lane reads per tap and half): at that kernel's budget its longest dispatch
    // (0.16 s, profiles/auto_lbda_device.txt) would pass 0.25 s -- half the budget here (measured: profiles/long_hrf.txt)
    f64_form(1, 640, 48, 64, kExactLong, 32768, 2048, "_long", "%d-tap", "register form", "outside 1..%d taps"),
    // four waves, up to 48 taps: the residency of the four-wave search (two workgroups per compute unit by its register
    // reports), and a pass that carries 48 taps for 32 -- that search's budget divided by 1.5, rounded down to a multiple of
    // 1 024 (32768 / 1.5 = 21845 -> 21504)
    f64_form(641, 1280, 48, 64 * pb::SPLIT_WAVES, kExactSplitLong, 21504, 256 * 2, "_split_long",
             "four-wave %d-tap", "register form", "outside 1..%d taps"),
};
// the window rule of every form is the reference's default (the searches carry no other: pb::AUTO_WIND)
constexpr int F64_WIND = 6;
static_assert(F64_WIND == pb::AUTO_WIND, "one window for the solves and the searches");

// the entry of `form` that carries a call, or nullptr: the form's scans and taps, a known stop rule, the window rule at F64_WIND
const ExactEntry* pick_f64(int form, int N, int K, int stop_mode, int wind) {
  const F64FormDesc& d = kF64[form];
  if (N < d.n_min || N > d.n_max || K < 1 || K > d.k_max) return nullptr;
  if (stop_mode < PB_STOP_NONE || stop_mode > PB_STOP_WINDOW) return nullptr;
  if (stop_mode == PB_STOP_WINDOW && wind != F64_WIND) return nullptr;
  return pick_cheapest(d.tab, d.n_tab, N, K, d.per_lane);
}
// The default dispatch of pb_fista_solve_d: one wave per series, else four (`four_waves`: calls with the taps on the host
// only -- pb_fista_solve_pp_d never falls through to four waves, PB_FLAG_PP_SPLIT names them); another window than F64_WIND
// has no register form.  The stop_mode is the caller's to validate: pb_fista_which_kernel_d / _pp_d pass an unknown one
// through and are answered as for a call without a rule.
const ExactEntry* pick_f64_default(int N, int K, int stop_mode, int wind, bool four_waves, int* form = nullptr) {
  if (stop_mode == PB_STOP_WINDOW && wind != F64_WIND) return nullptr;
  for (int f : {F64_ONE_WAVE, F64_FOUR_WAVES}) {
    const ExactEntry* e = (f == F64_ONE_WAVE || four_waves) ? pick_f64(f, N, K, PB_STOP_NONE, wind) : nullptr;
    if (e) {
      if (form) *form = f;
      return e;
    }
  }
  return nullptr;
}

template <int S, int KT>
constexpr launch_fn pair_or_null() {
  if constexpr (S <= 20 && KT <= 32) return &pb::launch_pair<S, KT>; else return nullptr;
}
template <int S, int KT>
constexpr launch_fn pair_ffa_or_null() {
  if constexpr (S <= 20 && KT <= 32) return &pb::launch_pair_ffa<S, KT>; else return nullptr;
}
template <int S, int KT>
constexpr int (*pair_dev_or_null())(const pb::FistaArgs&, hipStream_t) {
  if constexpr (S <= 20 && KT <= 32) return &pb::launch_pair_ffa_dev<S, KT>; else return nullptr;
}
template <int S, int KT>
constexpr pair_cert_fn pair_cert_or_null() {
  if constexpr (S <= 20 && KT <= 32) return &pb::launch_pair_ffa_cert<S, KT>; else return nullptr;
}
template <int S, int KT>
constexpr pair_split_fn pair_split_or_null() {
  if constexpr (S <= 20 && KT <= 32) return &pb::launch_pair_ffa_split<S, KT>; else return nullptr;
}
#define PB_FAST(S, KT)                                                                             \
  {S, KT, &pb::launch_fast<S, KT>, &pb::launch_fast_pp<S, KT>, pair_or_null<S, KT>(),             \
   pair_ffa_or_null<S, KT>(), pair_dev_or_null<S, KT>(), pair_cert_or_null<S, KT>(),              \
   pair_split_or_null<S, KT>()},
const FastEntry kFast[] = {
#include "fast_table.inc"
};
#undef PB_FAST

const FastEntry* pick_fast(int N, int K) { return pick_cheapest(kFast, N, K, 16); }

// series of 16 S < N <= 32 S scans: the pair form with the series' two halves in the slots of a row
const FastEntry* pick_split(int N, int K) {
  const FastEntry* best = nullptr;
  const FastEntry* whole = pick_fast(N, K);
  if (whole && whole->fn_pair_ffa) return nullptr;      // the series fits a slot: two PROBLEMS per row
  for (const FastEntry& e : kFast) {
    if (!e.fn_pair_split || e.KT < K || N <= 16 * e.S || N > 32 * e.S) continue;
    if (!best || (int64_t)e.S * e.KT < (int64_t)best->S * best->KT) best = &e;
  }
  return best;
}
// below this many series the one-problem-per-wave / single-row forms finish first (latency-bound)
constexpr int SPLIT_MIN_P = 1024;

// Plain solves (no stop rule) of a shape the matrix-pipe form serves AND some vector form can back up
// (remainders, re-solves of what its guards hand back): they go to the matrix pipe before the split-pair form
// is considered -- 305..310 scans fit ten blocks of 31 samples but have no single-slot pair entry, and one
// matrix-pipe wave beats the pair form over two slots.
bool mfma_serves_plain(int N, int K) {
  return pick_mfma(N, K, false) != nullptr && (pick_fast(N, K) != nullptr || pick_wide(N, K) != nullptr);
}
// without a single-row entry (305..310 scans and more than 32 taps) the remainder of the whole rounds goes to the
// one-problem-per-wave form when it is small, else everything runs on the matrix pipe (a partial last pass)
double wave_slots();
int mfma_wide_base(int P, bool one_launch) {
  const int round = (int)wave_slots() * 8;
  const int base = (P / round) * round;
  return (one_launch || P - base > round / 4) ? P : base;
}

// ---- launch plans: plan.h (host + device); here the host-side wrappers with this device's wave slots --------
using pb::Piece;
using pb::FORM_GENERIC; using pb::FORM_FAST1; using pb::FORM_PAIR; using pb::FORM_WIDE; using pb::FORM_MFMA; using pb::FORM_MFMA2;
using pb::MFMA2_BESIDE_CHUNKS;

double wave_slots() {
  static const double slots = [] {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess)
      return 2048.0;
    return (double)prop.multiProcessorCount * 4.0 * 2.0;
  }();
  return slots;
}
int best_form(int P, bool has_pair, bool has_wide, double* cost = nullptr) { return pb::best_form(P, has_pair, has_wide, wave_slots(), cost); }
int plan_pieces(int P, bool has_pair, bool has_wide, bool one_launch, bool one_stream, Piece* out) {
  return pb::plan_pieces(P, has_pair, has_wide, one_launch, one_stream, wave_slots(), out);
}
// ... for series of ten blocks; shorter series take one chunk at most: a pass of the one-wave form is cheaper for them
// relative to a chunk (round 4, sum-slot kernel: N = 240, 10 000 problems 1.36 ms as split pass + two chunks against
// 1.21 ms as one pass of the one-wave form; N = 300: 1.52 against 1.59 -- profiles/r4_split_form_passes.txt)
inline int beside_chunks_for(int N) { return N > 9 * pb::MFMA_SPAN ? MFMA2_BESIDE_CHUNKS : 1; }
// Series of 311 .. 640 scans (10 .. 20 blocks) run on the split form from this many problems on (below, the
// pair form over two slots or the latency-bound one-problem-per-wave form finish first: N = 600, 4 096 problems
// 1.58 ms against 1.93, 8 192 2.87 against 1.97 -- profiles/r4_split_form_passes.txt); whole passes of 8 192
// problems, a remainder above 5/16 of a pass too, a smaller one on the one-problem-per-wave form.
constexpr int MFMA2_LONG_MIN_P = 5120;
// (HRFs of 34+ taps have no pair form to compete with, and the one-problem-per-wave form pays for every tap: N = 600, K = 42,
// 4 096 problems 2.31 ms on the split form against 4.61 -- profiles/r5_long_series_42_taps.txt)
inline int mfma2_long_min_p(int K) { return K > 33 ? 2048 : MFMA2_LONG_MIN_P; }
bool mfma2_serves_long(int N, int K) { return N > MFMA1_NMAX && pick_mfma2(N, K, false) != nullptr && pick_wide(N, K) != nullptr; }
// 225 .. 310 scans with 34+ taps and the window rule: the one-wave form has no certificate beside three near tiles (its state does
// not fit), the split form has -- it takes such calls like a long series
bool mfma2_takes_short_cert(int N, int K, int stop_mode, int wind) {     // (... and the _loops_deconv rule, which the one-wave form lacks there too)
  return K > 33 && ((stop_mode == PB_STOP_WINDOW && wind == 6) || stop_mode == PB_STOP_LOOPS) && N > 224 && N <= MFMA1_NMAX &&
         pick_mfma2(N, K, false) != nullptr && pick_wide(N, K) != nullptr;
}
int mfma2_long_base(int P, bool one_launch) {
  const int pass = (int)wave_slots() * 4;            // 16 problems x (slots / 2 SIMDs / 2 waves)
  const int base = (P / pass) * pass;
  return (one_launch || P - base > pass * 5 / 16) ? P : base;
}
// Series of 641 .. 1 280 scans on the four-wave form: a pass is 16 problems per compute unit (4 096 on 256 of them) whatever
// the batch; whole passes, a remainder above MFMA4_MIN_R of a pass too, a smaller one -- and batches below it -- on the
// one-problem-per-wave form
constexpr int MFMA4_MIN_R_NUM = 10, MFMA4_MIN_R_DEN = 16;   // (N = 1 200: 2 048 problems 1.89 ms against 2.31, 3 072 2.59 against 2.30 -- profiles/r5_long_series_1200_scans.txt)
bool mfma4_serves(int N, int K) { return pick_mfma4(N, K, false) != nullptr && pick_wide(N, K) != nullptr; }
int mfma4_base(int P, bool one_launch) {
  const int pass = (int)wave_slots() * 2;            // 16 problems x (slots / 2 per SIMD / 4 SIMDs per workgroup)
  const int base = (P / pass) * pass;
  return (one_launch || (int64_t)(P - base) * MFMA4_MIN_R_DEN > (int64_t)pass * MFMA4_MIN_R_NUM) ? P : base;
}
int plan_pieces_mfma(int P, bool has_pair, bool has_wide, bool one_launch, bool one_stream, bool has_mfma2, int beside_chunks, Piece* out) {
  return pb::plan_pieces_mfma(P, has_pair, has_wide, one_launch, one_stream, has_mfma2, beside_chunks, wave_slots(), out);
}

// coherence bounds of the conditioning guard (path.h: path_class; calibrated on 5 120 series per length,
// profiles/r5_gamma_calibration_*.txt: above them the matrix-pipe form holds 3.3e-6 and the float32 vector forms 3e-6)
constexpr double PART_GAMMA_F64 = 1.0e-2, PART_GAMMA_MATRIX_PIPE = 7.0e-2;
// The bound below which a series stays off the matrix pipe, by shape: the error of the matrix-pipe forms at a given coherence falls
// with the length of the series (profiles/r5_gamma_calibration_*.txt, worst over the adversarial families per bin of gamma_2:
// 300 scans 4.8e-6 in [5e-2, 7e-2) and 6.7e-6 below; 600 scans 3.7e-6 in [3e-2, 5e-2), 4.9e-6 in [2e-2, 3e-2); 1 200 scans 5.4e-6 in
// [2e-2, 3e-2), 4.5e-6 in [1e-2, 2e-2); with 34+ taps 8.2e-6 in [5e-2, 7e-2) at 300 scans) -- and white noise, whose own error is
// 2e-6 at most, has a median gamma_2 of 6e-2 / 4e-2 / 3e-2 at 300 / 600 / 1 200 scans: one bound for every length kept nearly
// every noise-like series of 1 200 scans on the vector forms.
inline double part_gamma_matrix_pipe(int N, int K) {
  if (K > 33 || N <= 310) return PART_GAMMA_MATRIX_PIPE;
  return N <= 640 ? 3.0e-2 : 2.0e-2;
}
// below this many problems a call is latency-bound and keeps the host-side plan (a partition costs ~8 small launches)
constexpr int PART_MIN_P = 4096;

// the one-problem-per-wave entry worth using for SHORT series (the cheapest-per-problem tail
// form): only entries whose strips are at most 8 samples
const WideEntry* pick_wide_small(int N, int K) {
  const WideEntry* we = pick_wide(N, K);
  return (we && we->S <= 8) ? we : nullptr;
}

// Flag masks of the dispatch.  The forms split over waves, and the one-wave matrix-pipe form beside them, stay off under
// a pinned vector form or PB_FLAG_NO_MFMA
constexpr unsigned FLAGS_VECTOR_ONLY = PB_FLAG_FORCE_GENERIC | PB_FLAG_NO_PAIR | PB_FLAG_FORCE_PAIR | PB_FLAG_FORCE_WIDE |
                                       PB_FLAG_DIRECT_FIR | PB_FLAG_NO_MFMA;
// ... the one-wave matrix-pipe form as a piece of a single-row entry's plan (whose entry PB_FLAG_FORCE_GENERIC / _FORCE_WIDE
// have already ruled out); plan_ex reads these flags as "the plan without the matrix pipe"
constexpr unsigned FLAGS_PAIR_PIN_OR_NO_MFMA = PB_FLAG_NO_PAIR | PB_FLAG_FORCE_PAIR | PB_FLAG_DIRECT_FIR | PB_FLAG_NO_MFMA;
// the split pair form (one series over the two slots of a row)
constexpr unsigned FLAGS_NO_SPLIT_PAIR = PB_FLAG_FORCE_GENERIC | PB_FLAG_NO_PAIR | PB_FLAG_FORCE_WIDE | PB_FLAG_DIRECT_FIR;
// the partition on the device
constexpr unsigned FLAGS_NO_PARTITION = PB_FLAG_FORCE_GENERIC | PB_FLAG_FORCE_PAIR | PB_FLAG_FORCE_WIDE | PB_FLAG_NO_PAIR |
                                        PB_FLAG_DIRECT_FIR | PB_FLAG_NO_MFMA | PB_FLAG_ONE_LAUNCH | PB_FLAG_FORCE_MFMA2 |
                                        PB_FLAG_CERT_NO_RESOLVE | PB_FLAG_NO_PARTITION;

// ---- the route of pb_fista_solve_grouped (one HRF per parcel): the entry point runs it, pb_fista_grouped_route reports it ------
// Below this many rows a grouped call of 129 .. 310 scans stays on the per-problem vector route: a matrix-pipe pass costs the
// same whatever it carries (one wave per SIMD: 1.74 ms per 500 iterations at 300 scans), one problem per wave finishes up to
// 2 048 rows in 0.37 ms, and the per-problem route runs at 0.45 .. 0.6e9 row-iterations/s beyond: the pass wins
// from ~4 000 rows on.  (From those figures; not measured for grouped calls.)
constexpr int GROUPED_MFMA_MIN_P = 4096;
// the split forms of the grouped z-step (PB_FLAG_GROUPED_SPLIT): 311 .. 640 scans on two waves per unit, 641 .. 1 280 on four;
// up to 48 taps, where the table of the one-problem-per-wave form ends -- the rows behind the passes and the re-solve of
// handed-back rows need a vector form with per-row taps
constexpr int GROUPED_SPLIT_KMAX = 48;
grouped_launch_fn pick_mfma2_grouped(int N, int K) {
  static const grouped_launch_fn tab[] = {
      &pb::launch_mfma2_grouped<5, 5>, &pb::launch_mfma2_grouped<5, 6>, &pb::launch_mfma2_grouped<6, 6>, &pb::launch_mfma2_grouped<6, 7>,
      &pb::launch_mfma2_grouped<7, 7>, &pb::launch_mfma2_grouped<7, 8>, &pb::launch_mfma2_grouped<8, 8>, &pb::launch_mfma2_grouped<8, 9>,
      &pb::launch_mfma2_grouped<9, 9>, &pb::launch_mfma2_grouped<9, 10>, &pb::launch_mfma2_grouped<10, 10>};
  if (N <= MFMA1_NMAX || N > 640 || K < 1 || K > GROUPED_SPLIT_KMAX || !pick_wide(N, K)) return nullptr;
  return tab[(N + 31) / 32 - 10];
}
grouped_launch_fn pick_mfma4_grouped(int N, int K) {
  static const grouped_launch_fn tab[] = {&pb::launch_mfma4_grouped<6>, &pb::launch_mfma4_grouped<7>, &pb::launch_mfma4_grouped<8>,
                                          &pb::launch_mfma4_grouped<9>, &pb::launch_mfma4_grouped<10>};
  if (N <= 640 || N > 1280 || K < 1 || K > GROUPED_SPLIT_KMAX || !pick_wide(N, K)) return nullptr;
  return tab[(N + 127) / 128 - 6];
}

// `code`: the main launch in the numbering of pb_fista_which_kernel -- 4 one wave per unit of 16 rows, 5 two waves, 6 four
// waves, 0 every row on the per-problem vector route, -1 the flags force a form the shape lacks; `main_units`: the units of
// the table in that launch (from the first on); `row_cut`: the first row behind them (P: none) -- those rows run on the
// vector forms.  code 0: main_units = 0, row_cut = 0.
struct GroupedRoute {
  int code, main_units, row_cut;
  grouped_launch_fn fn;
};
// first row of unit `whole` of the table (units of GROUPED_WAVE_ROWS rows that never cross a parcel)
int grouped_row_of_unit(const int32_t* offsets_host, int G, int P, int whole) {
  int u = 0;
  for (int g = 0; g < G; ++g) {
    const int n = (offsets_host[g + 1] - offsets_host[g] + pb::GROUPED_WAVE_ROWS - 1) / pb::GROUPED_WAVE_ROWS;
    if (u + n > whole) return offsets_host[g] + (whole - u) * pb::GROUPED_WAVE_ROWS;
    u += n;
  }
  return P;
}
// (offsets checked by the caller, P > 0; `n_done`: n_done_dev given -- the matrix-pipe forms hand rows back through it)
GroupedRoute route_grouped(const int32_t* offsets_host, int G, int P, int N, int K, unsigned fl, bool n_done) {
  GroupedRoute r{0, 0, 0, nullptr};
  const bool forced = (fl & PB_FLAG_FORCE_MFMA) != 0, one_launch = forced || (fl & PB_FLAG_ONE_LAUNCH) != 0;
  const bool pipe = n_done && !(fl & FLAGS_VECTOR_ONLY);
  const bool split = (fl & PB_FLAG_GROUPED_SPLIT) != 0 && N > MFMA1_NMAX;      // (up to 310 scans the flag changes nothing)
  const bool four = N > 640;
  r.fn = !pipe ? nullptr : !split ? pick_mfma_grouped(N, K) : four ? pick_mfma4_grouped(N, K) : pick_mfma2_grouped(N, K);
  if (!r.fn) {
    r.code = forced ? -1 : 0;
    return r;
  }
  const int units = pb::grouped_table(offsets_host, G, P, pb::GROUPED_WAVE_ROWS, nullptr, nullptr);
  int main_units = units;
  if (!split) {
    // Whole rounds of waves (one per SIMD) go to the matrix pipe; a last partial round costs a whole pass there whatever it
    // carries, so up to GROUPED_MFMA_MIN_P rows of it go to the vector forms instead, behind the rounds (the split of
    // plan_pieces_mfma; not under PB_FLAG_ONE_LAUNCH / _FORCE_MFMA)
    if (!forced && P < GROUPED_MFMA_MIN_P) main_units = 0;
    else if (!one_launch) {
      const int round = (int)wave_slots() / 2;
      const int whole = units / round * round;
      if (whole > 0 && whole < units && P - grouped_row_of_unit(offsets_host, G, P, whole) <= GROUPED_MFMA_MIN_P) main_units = whole;
    }
  } else if (!forced) {
    // The thresholds of the shared-HRF route (route_pp: mfma2_long_min_p, mfma2_long_base, mfma4_base) applied to 16 x units,
    // because a unit costs a workgroup whatever it carries: whole passes on the matrix pipe, a remainder above 5/16 (two waves)
    // or 10/16 (four waves) of a pass too, a smaller one behind the passes on the vector forms.  MEASURED FOR THE SHARED-HRF
    // FORMS, not for grouped calls (profiles/r4_split_form_passes.txt, r5_long_series_*.txt; profiles/parcels_split.txt says
    // what is known about grouped ones).  A two-wave call that meets the minimum but fills no whole pass is one partial pass:
    // there the minimum decides, not the remainder rule (34+ taps, 2 048 .. 2 560 rows).
    const int slot_rows = 16 * units;
    if (!four && slot_rows < mfma2_long_min_p(K)) main_units = 0;
    else {
      const int base = (four ? mfma4_base(slot_rows, one_launch) : mfma2_long_base(slot_rows, one_launch)) / 16;
      main_units = (!four && base == 0) ? units : base;
    }
  }
  if (main_units == 0) {
    r.fn = nullptr;
    return r;
  }
  r.code = !split ? 4 : four ? 6 : 5;
  r.main_units = main_units;
  r.row_cut = main_units == units ? P : grouped_row_of_unit(offsets_host, G, P, main_units);
  return r;
}

// The window rule at the reference's wind = 6 as a per-iteration no-fire certificate (fista_pair_ffa.h, the matrix-pipe
// forms), then an exact re-solve of the problems it could not clear (n_done = -1).  Worth it when the rule is not expected
// to fire: the criterion decays like ~0.9/k on this problem class, so it cannot pass below tol before k ~ 0.9/tol --
// tol * n_iter < CERT_TN_VECTOR.  The matrix-pipe forms' bound rests on four tracked samples per problem instead of
// sixteen: only where the rule is far from firing, tol * n_iter < CERT_TN_MATRIX_PIPE; closer calls stay on the pair form.
constexpr double CERT_TN_VECTOR = 0.5, CERT_TN_MATRIX_PIPE = 0.02;

// ---- the dispatch of a float32 call: pb_fista_solve runs its route, the queries report it -------------------------------
struct Call {
  int N, K, P, stop_mode, wind;
  unsigned flags;
  bool cost_trace;     // J_dev given
  bool lbda_vec;       // one lambda per problem
  bool n_done;         // n_done_dev given
  double tol_iters;    // tol * n_iter
  bool taps_dev;       // the taps in device memory too
  bool workspace;      // a partition workspace can be used
  bool reported;       // a query: the cells where the queries have always answered otherwise than the solve runs (below)
};

enum Path {
  PATH_PART_LONG,      // 311 .. 1 280 scans partitioned on the device: a split matrix-pipe form, the split pair form, the backup form
  PATH_SPLIT_LONG,     // whole passes of a split matrix-pipe form, the remainder and the re-solve on the backup form
  PATH_SPLIT_PAIR,     // the pair form with the two halves of ONE series in the slots of a row
  PATH_PART_SHORT,     // a single-row entry's shape partitioned on the device: the one-wave matrix-pipe form and vector forms
  PATH_PIECES,         // the host-side plan of a single-row entry's shape (plan.h), or one pinned form
  PATH_MFMA_WIDE,      // the one-wave matrix-pipe form beside the one-problem-per-wave form
  PATH_WIDE,           // one problem per wave
  PATH_GENERIC         // the any-size LDS kernel
};

struct Route {
  Path path;
  const FastEntry* fe;   // single-row entry: PIECES, PART_SHORT; the backup form of SPLIT_LONG / PART_LONG unless backup_wide
  const WideEntry* we;   // one-problem-per-wave entry: WIDE, MFMA_WIDE, SPLIT_PAIR's re-solve, the backup form when backup_wide;
                         // PIECES, PART_SHORT: the entry for short series (pick_wide_small) or nullptr
  const FastEntry* se;   // split pair entry: SPLIT_PAIR, PART_LONG
  launch_fn mfma;        // one-wave matrix-pipe form: PIECES, PART_SHORT, MFMA_WIDE (PART_SHORT without it: no dense class)
  launch_fn split;       // the form split over two waves (over four beyond 640 scans)
  bool backup_wide;
  bool cert;             // the window rule as a certificate on the pair form (SPLIT_PAIR, PART_LONG: the split pair form)
  bool mfma_cert;        // ... on the one-wave matrix-pipe form too
  bool has_pair, has_wide, has_mfma2;   // the forms a plan may use (PART_LONG: has_pair = the split pair form)
  int one_form;          // PIECES: this form over every problem in one launch (0: the plan)
  int base;              // SPLIT_LONG, MFMA_WIDE: problems [0, base) on the matrix-pipe form
  int beside_chunks;     // PIECES: chunks of one-problem waves the plan may put beside a pass of the split form
  bool one_stream;       // PIECES: the plan stays on the caller's stream whatever the flags say
};

Route route(const Call& c) {
  const int N = c.N, K = c.K, P = c.P, stop = c.stop_mode;
  const unsigned fl = c.flags;
  const bool plain = stop == PB_STOP_NONE, window6 = stop == PB_STOP_WINDOW && c.wind == 6;
  Route r{};
  const bool part_ws = c.workspace && c.n_done && P >= PART_MIN_P && K <= pb::LMAX_KT && N <= 1280 && !(fl & FLAGS_NO_PARTITION);
  // the window rule as a certificate on a form with this limit of tol * n_iter
  auto cert_clears = [&](double limit) { return !(fl & PB_FLAG_NO_CERT) && ((fl & PB_FLAG_FORCE_CERT) || c.tol_iters < limit); };
  // the split matrix-pipe forms: plain solves, the certificate, the _loops_deconv rule in full inside the kernel (no cost
  // trace); one lambda per problem only when asked for
  const bool split_cert = window6 && c.n_done && cert_clears(CERT_TN_MATRIX_PIPE);
  const bool split_rule = plain || split_cert || (stop == PB_STOP_LOOPS && !c.cost_trace);
  const bool split_shape = split_rule && c.n_done && !(fl & FLAGS_VECTOR_ONLY) &&
                           (!c.lbda_vec || (fl & (PB_FLAG_FORCE_MFMA | PB_FLAG_FORCE_MFMA2)));
  const launch_fn mfma2 = split_shape ? pick_mfma2(N, K, false) : nullptr;
  const launch_fn mfma4 = (split_shape && mfma4_serves(N, K)) ? pick_mfma4(N, K, false) : nullptr;
  const bool four = N > 640;
  const bool long_shape = mfma2_serves_long(N, K) || mfma2_takes_short_cert(N, K, stop, c.wind);
  const bool long_call = long_shape && P >= mfma2_long_min_p(K);
  // the exact vector form behind a split form (remainder, re-solve): single row, else one per wave -- with the window rule it
  // must hold the rule's increment ring (the queries check the one-problem-per-wave entry's: 311..320 scans)
  const FastEntry* fe1 = pick_fast(N, K);
  const WideEntry* we1 = pick_wide(N, K);
  r.backup_wide = we1 && (!fe1 || N > 320);
  const bool backup_ok = (fe1 || we1) && ring_fits((r.backup_wide || (c.reported && we1)) ? we1->S : fe1->S, stop, c.wind);
  // series of 16 S < N <= 32 S scans (the reference's 600-scan demo): the pair form with the two halves of ONE series in the
  // slots of a row; the window rule as a certificate, re-solved on the one-problem-per-wave form
  r.se = pick_split(N, K);
  const bool split_pair_cert = r.se && window6 && c.n_done && we1 && ring_fits(we1->S, stop, c.wind) && cert_clears(CERT_TN_VECTOR);

  // 311 .. 1 280 scans partitioned on the device: the dense class on whole passes of the split form, the sparse class on the
  // pair form over two slots (or the backup form), handed-back problems compacted
  if (part_ws && split_rule && (four ? mfma4_serves(N, K) : long_call) && backup_ok) {
    r.path = PATH_PART_LONG;
    r.split = four ? pick_mfma4(N, K, false) : pick_mfma2(N, K, false);
    r.fe = fe1;
    r.we = we1;
    r.cert = split_pair_cert;
    r.has_pair = r.se && (plain || split_pair_cert);
    return r;
  }
  // Series of 311 .. 640 scans on the two-wave split form from mfma2_long_min_p problems on, 641 .. 1 280 on the four-wave
  // form: whole passes (and a large remainder), the rest and whatever its guards hand back on the backup form.  Shorter
  // series meet the two-wave form as a piece of the plan below (small batches, remainders) or through PB_FLAG_FORCE_MFMA2.
  // (PB_FLAG_FORCE_MFMA2 as the queries report it: the long shapes, and plain solves or the certificate with up to 33 taps
  // whatever the backup form)
  const bool forced = (fl & PB_FLAG_FORCE_MFMA2) != 0;
  const bool forced_short = c.reported && forced && (plain || window6) && pick_mfma2(N, K, true);
  const launch_fn split = mfma4 ? mfma4 : ((mfma2 && ((forced && (!c.reported || long_shape || forced_short)) || long_call)) ? mfma2 : nullptr);
  if (split && (backup_ok || forced_short)) {
    r.path = PATH_SPLIT_LONG;
    r.split = split;
    r.fe = fe1;
    r.we = we1;
    const bool one_launch = (fl & PB_FLAG_ONE_LAUNCH) != 0;
    r.base = (fl & PB_FLAG_FORCE_MFMA2) ? P : (mfma4 ? mfma4_base(P, one_launch) : mfma2_long_base(P, one_launch));
    return r;
  }
  const bool mfma_plain = plain && c.n_done && (!c.lbda_vec || (fl & PB_FLAG_FORCE_MFMA)) && !(fl & FLAGS_VECTOR_ONLY) &&
                          mfma_serves_plain(N, K);
  if (!mfma_plain && !(fl & FLAGS_NO_SPLIT_PAIR) && r.se && (P >= SPLIT_MIN_P || (fl & PB_FLAG_FORCE_PAIR)) &&
      (plain || split_pair_cert)) {
    r.path = PATH_SPLIT_PAIR;
    r.we = we1;
    r.cert = split_pair_cert;
    return r;
  }
  // the register-resident window rule keeps wind-1 iterates: wind = 4, 6 or 8 on entries small enough to hold them
  const FastEntry* fe = (fl & (PB_FLAG_FORCE_GENERIC | PB_FLAG_FORCE_WIDE)) ? nullptr : fe1;
  if (fe && !ring_fits(fe->S, stop, c.wind)) fe = nullptr;
  if (fe) {
    r.fe = fe;
    // (the queries report the certificate for a single problem too)
    r.cert = window6 && fe->fn_pair_cert && c.n_done && (P >= 2 || c.reported) && !(fl & (PB_FLAG_NO_PAIR | PB_FLAG_DIRECT_FIR)) &&
             cert_clears(CERT_TN_VECTOR);
    // Plain solves (cost trace or not) of 129..310 scans, HRFs up to 33 taps (34..65: plain solves only): both operators on
    // the matrix pipe (fista_mfma.h).  Needs n_done_dev: a problem whose scaled operands left the float16 range comes back
    // with n_done = -1 and is re-solved on the single-row form.  Not with one lambda per problem, unless asked for
    // (PB_FLAG_FORCE_MFMA): along a regularisation path a third of the problems (lambda near lambda_max) fail that
    // kernel's accuracy guard and would be solved twice.  The window rule rides it as the certificate; the _loops_deconv
    // rule is evaluated exactly inside it (no cost trace, K <= 33).
    r.mfma_cert = r.cert && ((fl & PB_FLAG_FORCE_MFMA) || c.tol_iters < CERT_TN_MATRIX_PIPE);
    const bool mfma_rule = plain || r.mfma_cert || (stop == PB_STOP_LOOPS && !c.cost_trace && K <= MFMA_K2);
    const launch_fn mfma_shape = mfma_rule ? pick_mfma(N, K, !plain, (fl & PB_FLAG_MFMA_DENSE_TILES) != 0) : nullptr;
    const launch_fn mfma = (mfma_shape && c.n_done && (!c.lbda_vec || (fl & PB_FLAG_FORCE_MFMA)) && !(fl & FLAGS_PAIR_PIN_OR_NO_MFMA))
                               ? mfma_shape : nullptr;
    r.has_pair = (fe->fn_pair && plain) || r.cert;
    r.we = pick_wide_small(N, K);
    r.has_wide = r.we != nullptr;
    r.beside_chunks = beside_chunks_for(N);
    r.path = PATH_PIECES;
    if (fl & PB_FLAG_NO_PAIR) {
      r.one_form = FORM_FAST1;
      return r;
    }
    // A call no matrix-pipe form carries -- another window, a cost trace beside the _loops_deconv rule, a long HRF -- is
    // partitioned all the same, with an empty dense class: the conditioning guard is the partition's, and float32 vector
    // forms need it too (ill-conditioned series: 3e-5 .. 5e-3 without it)
    const bool part_mfma = mfma || (c.lbda_vec && mfma_shape);
    if (part_ws && (part_mfma || !(fl & PB_FLAG_NO_ILL_GUARD))) {
      r.path = PATH_PART_SHORT;
      r.mfma = part_mfma ? mfma_shape : nullptr;
      r.split = !part_mfma ? nullptr
                : (mfma2 || !c.lbda_vec) ? mfma2
                : ((plain || split_cert) && K <= MFMA_K2) ? pick_mfma2(N, K, false) : nullptr;
      r.has_mfma2 = r.split && (plain || r.mfma_cert);
      return r;
    }
    r.mfma = mfma;
    r.split = mfma2;
    // (the queries plan the two-wave form with up to 33 taps)
    r.has_mfma2 = c.reported ? (plain || window6) && pick_mfma2(N, K, true) : mfma2 && (plain || r.mfma_cert);
    if (fl & PB_FLAG_FORCE_PAIR) r.one_form = (r.cert || (fe->fn_pair && P >= 2 && plain)) ? FORM_PAIR : FORM_FAST1;
    return r;
  }
  // 305..310 scans with more than 32 taps: no single-row entry, but ten blocks of 31 samples fit the matrix-pipe form --
  // whole rounds (or everything) on it, a small remainder and the problems its guards hand back on the one-problem-per-wave form
  const launch_fn mf = mfma_plain ? pick_mfma(N, K, false, (fl & PB_FLAG_MFMA_DENSE_TILES) != 0) : nullptr;
  if (mf && we1) {
    r.path = PATH_MFMA_WIDE;
    r.mfma = mf;
    r.we = we1;
    r.base = mfma_wide_base(P, (fl & PB_FLAG_ONE_LAUNCH) != 0);
    return r;
  }
  // long series: one problem per wave
  if (!(fl & PB_FLAG_FORCE_GENERIC) && we1 && ring_fits(we1->S, stop, c.wind)) {
    r.path = PATH_WIDE;
    r.we = we1;
    return r;
  }
  r.path = PATH_GENERIC;
  return r;
}

// The route of pb_fista_solve_pp (taps and steps in device memory; no stop rule, or the _loops_deconv rule): never partitioned,
// always on the caller's stream.  ONE shared HRF without a stop rule takes the paths of a float32 call, the matrix-pipe and
// pair forms reading the HRF and its step from device memory: whole passes of a split form for 311 .. 1 280 scans (the rest
// and the re-solve one problem per wave), below that the plan of the single-row entry's forms -- with two beside-chunks
// whatever the length of the series.  One HRF per problem: the single-row form, or one problem per wave where that finishes
// first (small batches are latency-bound: 0.37 ms against 0.93 ms per 500 iterations up to 2 048).
Route route_pp(int N, int K, int P, bool shared, int stop_mode, bool n_done, unsigned fl) {
  Route r{};
  const bool plain_shared = shared && stop_mode == PB_STOP_NONE;
  const WideEntry* we1 = pick_wide(N, K);
  if (N > MFMA1_NMAX && plain_shared && n_done && K <= 65 && !(fl & FLAGS_VECTOR_ONLY)) {
    const bool four = N > 640;
    const launch_fn split = four ? pick_mfma4(N, K, false) : pick_mfma2(N, K, false);
    if (split && we1 && (four || P >= mfma2_long_min_p(K) || (fl & PB_FLAG_FORCE_MFMA2))) {
      const bool all = (fl & (PB_FLAG_ONE_LAUNCH | PB_FLAG_FORCE_MFMA2)) != 0;
      r.path = PATH_SPLIT_LONG;
      r.split = split;
      r.we = we1;
      r.backup_wide = true;
      r.base = four ? mfma4_base(P, all) : mfma2_long_base(P, all);
      return r;
    }
  }
  r.fe = (fl & PB_FLAG_FORCE_GENERIC) ? nullptr : pick_fast(N, K);
  if (r.fe) {
    r.path = PATH_PIECES;
    r.one_stream = true;
    r.we = pick_wide_small(N, K);
    r.has_wide = r.we != nullptr;
    if (plain_shared && r.fe->fn_pair_dev && P >= 2 && !(fl & (PB_FLAG_NO_PAIR | PB_FLAG_DIRECT_FIR))) {
      r.has_pair = true;
      r.beside_chunks = MFMA2_BESIDE_CHUNKS;
      if (fl & PB_FLAG_FORCE_PAIR) {
        r.one_form = FORM_PAIR;
        return r;
      }
      r.mfma = (n_done && !(fl & PB_FLAG_NO_MFMA)) ? pick_mfma(N, K, false, (fl & PB_FLAG_MFMA_DENSE_TILES) != 0) : nullptr;
      r.split = (r.mfma && K <= MFMA_K2) ? pick_mfma2(N, K, false) : nullptr;
      r.has_mfma2 = r.split != nullptr;
      return r;
    }
    const bool wide_first = r.we && !(fl & (PB_FLAG_NO_PAIR | PB_FLAG_FORCE_PAIR | PB_FLAG_ONE_LAUNCH)) && best_form(P, false, true) == FORM_WIDE;
    r.one_form = wide_first ? FORM_WIDE : FORM_FAST1;
    return r;
  }
  r.we = (fl & PB_FLAG_FORCE_GENERIC) ? nullptr : we1;
  r.path = r.we ? PATH_WIDE : PATH_GENERIC;
  return r;
}

// PATH_PIECES: the pinned form over every problem, else the plan of its forms (plan.h)
int route_pieces(const Route& r, int P, bool one_launch, bool one_stream, Piece* pc) {
  if (r.one_form) {
    pc[0] = Piece{r.one_form, 0, P, false, false};
    return 1;
  }
  if (r.mfma) return plan_pieces_mfma(P, r.has_pair, r.has_wide, one_launch, one_stream, r.has_mfma2, r.beside_chunks, pc);
  return plan_pieces(P, r.has_pair, r.has_wide, one_launch, one_stream, pc);
}

// What the queries report of a route: problems [0, n_main) on main_form, the rest (mostly) on tail_form.  Of pieces, the
// leading ones of one form are the "main" part, the first other form the tail (of several: the one that carries most
// of the remaining problems).  A partitioned call reports its host-side plan: the queries describe calls without a workspace.
void report(const Route& r, int N, int P, bool one_launch, bool one_stream, int* nm, int* mf, int* tf) {
  auto passes = [&](int base, int form, int rest) {
    if (base > 0 && base < P) { *nm = base; *mf = form; *tf = rest; }
    else *tf = base > 0 ? form : rest;
  };
  *nm = *mf = *tf = 0;
  switch (r.path) {
    case PATH_SPLIT_LONG: passes(r.base, N > 640 ? pb::FORM_MFMA4 : FORM_MFMA2, r.backup_wide ? FORM_WIDE : FORM_FAST1); return;
    case PATH_MFMA_WIDE: passes(r.base, FORM_MFMA, FORM_WIDE); return;
    case PATH_SPLIT_PAIR: *tf = FORM_PAIR; return;
    case PATH_WIDE: *tf = FORM_WIDE; return;
    case PATH_PIECES: {
      Piece pc[pb::MAX_PIECES];
      const int npc = route_pieces(r, P, one_launch, one_stream, pc);
      int i = 1;
      while (i < npc && pc[i].form == pc[0].form) ++i;
      if (i == npc) { *tf = pc[0].form; return; }
      *nm = pc[i - 1].p1;
      *mf = pc[0].form;
      int big = i;
      for (int k = i + 1; k < npc; ++k)
        if (pc[k].p1 - pc[k].p0 > pc[big].p1 - pc[big].p0) big = k;
      *tf = pc[big].form;
      return;
    }
    default: *tf = FORM_GENERIC; return;
  }
}

}  // namespace
