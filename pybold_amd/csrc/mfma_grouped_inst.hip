// The matrix-pipe z-step with one HRF per parcel (fista_mfma_grouped.h): series of 129..310 scans (NB blocks of 31
// samples + one sum slot), HRFs of up to 33 taps.
#include "fista_mfma_grouped.h"
#ifndef PB_NB
#error "compile with -DPB_NB=<blocks of 31 samples>"
#endif
namespace pb {
template int launch_mfma_grouped<PB_NB>(const FistaArgs&, int, hipStream_t);
}
