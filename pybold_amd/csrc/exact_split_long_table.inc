// (S samples per lane, KT taps) specialisations of the all-float64 one-problem-per-workgroup (four waves) kernels with the
// taps in one VGPR pair of every wave (fista_exact_split_long.h): series of up to 4*64*S scans, HRFs of up to KT <= 64
// taps.  OPT-IN: a table of its own -- pick_exact, pick_auto_split and pick_exact_split_pp read exact_split_table.inc and
// never come here.
PB_EXACT_SPLIT_LONG(5, 48)
