// The plain matrix-pipe solve on 2:4-sparse near tiles (fista_mfma_sparse.h): series of 129..310 scans, HRFs of up to
// 32 taps; every other call of the one-wave form goes on to mfma_inst.hip's variants.
#include "fista_mfma_sparse.h"
#ifndef PB_NB
#error "compile with -DPB_NB=<blocks of 31 samples>"
#endif
namespace pb {
extern template int launch_mfma<PB_NB>(const FistaArgs&, const double*, int, bool, hipStream_t);
template int launch_mfma_st<PB_NB>(const FistaArgs&, const double*, int, bool, hipStream_t);
}
