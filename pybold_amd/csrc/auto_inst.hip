// One (PB_S, PB_KT) specialisation of the device-resident lambda search (fista_auto.h), from exact_table.inc.
#include "fista_auto.h"
#ifndef PB_S
#error "compile with -DPB_S=<samples per lane> -DPB_KT=<taps>"
#endif
namespace pb {
template int launch_auto<PB_S, PB_KT>(const AutoArgs&, const double*, int, bool, hipStream_t);
}
