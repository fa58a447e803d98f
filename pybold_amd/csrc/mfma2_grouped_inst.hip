// The two-wave matrix-pipe z-step with one HRF per parcel (fista_mfma_split_grouped.h): series of 289 .. 640 scans
// (NBA + NBB blocks of 32 samples; the route sends 311 .. 640 here), HRFs of up to 33 taps on two near tiles, longer ones on three.
#include "fista_mfma_split_grouped.h"
#if !defined(PB_NBA) || !defined(PB_NBB)
#error "compile with -DPB_NBA=<blocks of the left wave> -DPB_NBB=<blocks of the right wave>"
#endif
namespace pb {
template int launch_mfma2_grouped<PB_NBA, PB_NBB>(const FistaArgs&, int, hipStream_t);
}
