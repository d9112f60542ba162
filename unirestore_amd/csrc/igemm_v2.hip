// Instantiation unit of the implicit-GEMM launchers (see igemm_impl.h); dispatched from igemm.hip.
#include "igemm_impl.h"

namespace urk {
UR_LAUNCHER(v2_256x32, Glds<256, 32, 4, 1, 3, 200>)
UR_LAUNCHER(v2_128x64, Glds<128, 64, 2, 2, 3, 200>)
UR_LAUNCHER(v2_256x160, Glds<256, 160, 8, 1, 3, 0>)
UR_LAUNCHER(v2_256x128, Glds<256, 128, 4, 2, 3, 0>)
UR_LAUNCHER(gemm_256x320_pair, Gemm<256, 320, 8, 1, 2, false, true>)
UR_LAUNCHER(gemm_256x256, Gemm<256, 256, 4, 2, 2>)
}  // namespace urk
