// One (PB_S, PB_KT) specialisation of the device-resident lambda search with one voxel over four waves
// (fista_auto_split.h), from exact_split_table.inc.
#include "fista_auto_split.h"
#ifndef PB_S
#error "compile with -DPB_S=<samples per lane> -DPB_KT=<taps>"
#endif
namespace pb {
template int launch_auto_split<PB_S, PB_KT>(const AutoArgs&, const double*, int, bool, hipStream_t);
}
