// Instantiation unit of the implicit-GEMM launchers (see igemm_impl.h); dispatched from igemm.hip.
#include "igemm_impl.h"

namespace urk {
UR_LAUNCHER(halo_8x32_160, Halo<8, 160, 8, 1>)
UR_LAUNCHER(halo_8x32_128, Halo<8, 128, 4, 2>)
UR_LAUNCHER(halo_thin_32, HaloThin<8, 32, 8, 1>)
UR_LAUNCHER(himg_16x16, HaloImg<16, 16, 1, 128, 4, 2>)
UR_LAUNCHER(himg_8x8x4, HaloImg<8, 8, 4, 128, 4, 2>)
}  // namespace urk
