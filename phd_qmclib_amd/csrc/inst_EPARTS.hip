// Explicit instantiations of the energy-parts kernel (qmc_energy_parts.h),
// translation unit EPARTS.
#include "qmc_energy_parts.h"
#define QMC_NO_KW
QMC_TU_EPARTS(QMC_NO_KW)
