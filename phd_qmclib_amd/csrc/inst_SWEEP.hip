// Explicit instantiations of the single-particle VMC sweeps
// (qmc_vmc_sweep.h), translation unit SWEEP.
#include "qmc_vmc_sweep.h"
#define QMC_NO_KW
QMC_TU_SWEEP(QMC_NO_KW)
