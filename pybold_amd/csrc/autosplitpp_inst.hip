// One (PB_S, PB_KT) specialisation of the device-resident lambda search with one HRF per voxel and one voxel over four
// waves (fista_exact_split_pp.h), from exact_split_table.inc.
#include "fista_exact_split_pp.h"
#ifndef PB_S
#error "compile with -DPB_S=<samples per lane> -DPB_KT=<taps>"
#endif
namespace pb {
template int launch_auto_split_pp<PB_S, PB_KT>(const AutoArgsPP&, bool, hipStream_t);
}
