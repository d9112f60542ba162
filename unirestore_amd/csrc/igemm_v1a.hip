// Instantiation unit of the implicit-GEMM launchers (see igemm_impl.h); dispatched from igemm.hip.
#include "igemm_impl.h"

namespace urk {
UR_LAUNCHER(v1_128x128, Cfg<128, 128, 2, 2>)
UR_LAUNCHER(v1_128x160, Cfg<128, 160, 4, 1>)
}  // namespace urk
