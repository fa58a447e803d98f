// (S samples per lane, KT taps) specialisations of the all-float64 kernel with one series over the four waves of a
// workgroup (fista_exact_split.h): series of up to 4*64*S scans, HRFs of up to KT taps.  A table of its own: the
// device-resident lambda search (fista_auto.h) reads exact_table.inc and has no four-wave form.
PB_EXACT_SPLIT(5, 32)
