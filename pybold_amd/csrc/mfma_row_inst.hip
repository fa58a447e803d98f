// One series per wave on the matrix pipe (fista_mfma_row.h): one kernel for 129 .. 320 scans and up to 33 taps.
#define PB_MFMA_ROW_INST
#include "fista_mfma_row.h"
