// One (PB_S, PB_KT) specialisation of the float64 solve with the taps in one VGPR pair (fista_exact_long.h),
// from exact_long_table.inc.
#include "fista_exact_long.h"
#ifndef PB_S
#error "compile with -DPB_S=<samples per lane> -DPB_KT=<taps>"
#endif
namespace pb {
template int launch_exact_long<PB_S, PB_KT>(const FistaArgs&, const double*, int, bool, int, hipStream_t);
}
