// Explicit instantiations of the second-order DMC step (qmc_evolve2.h),
// translation unit E2_64_2; see qmc_inst.h.
#include "qmc_inst.h"
QMC_TU_E2_64_2(QMC_NO_KW)
