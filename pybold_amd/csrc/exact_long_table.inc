// (S samples per lane, KT taps) specialisations of the all-float64 one-problem-per-wave kernels with the taps in one
// VGPR pair of the wave (fista_exact_long.h): series of up to 64*S scans, HRFs of up to KT <= 64 taps.  OPT-IN: a table
// of its own -- pick_exact, pick_auto and pick_exact_pp read exact_table.inc and never come here.
PB_EXACT_LONG(5, 48)
PB_EXACT_LONG(10, 48)
