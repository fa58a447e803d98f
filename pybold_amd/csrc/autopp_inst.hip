// One (PB_S, PB_KT) specialisation of the device-resident lambda search with one HRF per voxel (fista_exact_pp.h),
// from exact_table.inc.
#include "fista_exact_pp.h"
#ifndef PB_S
#error "compile with -DPB_S=<samples per lane> -DPB_KT=<taps>"
#endif
namespace pb {
template int launch_auto_pp<PB_S, PB_KT>(const AutoArgsPP&, bool, hipStream_t);
}
