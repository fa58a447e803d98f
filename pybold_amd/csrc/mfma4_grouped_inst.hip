// The four-wave matrix-pipe z-step with one HRF per parcel (fista_mfma_split_grouped.h): A blocks of 32 samples per wave,
// 128 (A - 1) < N <= 128 A; HRFs of up to 33 taps on two near tiles, longer ones on three.
#include "fista_mfma_split_grouped.h"
#if !defined(PB_A)
#error "compile with -DPB_A=<blocks per wave>"
#endif
namespace pb {
template int launch_mfma4_grouped<PB_A>(const FistaArgs&, int, hipStream_t);
}
