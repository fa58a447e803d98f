// One (PB_S, PB_KT) specialisation of the all-float64 register-resident kernel with one HRF per problem and one series
// over four waves (fista_exact_split_pp.h), from exact_split_table.inc.
#include "fista_exact_split_pp.h"
#ifndef PB_S
#error "compile with -DPB_S=<samples per lane> -DPB_KT=<taps>"
#endif
namespace pb {
template int launch_exact_split_pp<PB_S, PB_KT>(const FistaArgs&, bool, int, hipStream_t);
}
