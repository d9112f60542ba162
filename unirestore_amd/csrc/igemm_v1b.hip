// Instantiation unit of the implicit-GEMM launchers (see igemm_impl.h); dispatched from igemm.hip.
#include "igemm_impl.h"

namespace urk {
UR_LAUNCHER(v1_128x64, Cfg<128, 64, 2, 2>)
UR_LAUNCHER(v1_256x32, Cfg<256, 32, 4, 1>)
UR_LAUNCHER(v1_64x64, Cfg<64, 64, 2, 2>)
}  // namespace urk
