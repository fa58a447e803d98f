// One (PB_S, PB_KT) specialisation of the four-wave lambda search with one HRF per voxel, the taps in one VGPR pair of
// every wave (fista_exact_split_long.h), from exact_split_long_table.inc.
#include "fista_exact_split_long.h"
#ifndef PB_S
#error "compile with -DPB_S=<samples per lane> -DPB_KT=<taps>"
#endif
namespace pb {
template int launch_auto_split_long_pp<PB_S, PB_KT>(const AutoArgsPP&, bool, hipStream_t);
}
