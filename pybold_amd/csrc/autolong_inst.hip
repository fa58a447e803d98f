// One (PB_S, PB_KT) specialisation of the device-resident lambda search with the taps in one VGPR pair (fista_exact_long.h),
// from exact_long_table.inc.
#include "fista_exact_long.h"
#ifndef PB_S
#error "compile with -DPB_S=<samples per lane> -DPB_KT=<taps>"
#endif
namespace pb {
template int launch_auto_long<PB_S, PB_KT>(const AutoArgs&, const double*, int, bool, hipStream_t);
}
