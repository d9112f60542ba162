// Instantiation unit: pure-GEMM LDS-DMA kernels at the small tile shapes (two-stage ring, two or more workgroups per CU).
#include "igemm_impl.h"

// ring depth per tile shape (stages of the LDS-DMA K ring); -D overrides are for A/B builds
#ifndef UR_NST_128x128
#define UR_NST_128x128 2
#endif
#ifndef UR_NST_128x160
#define UR_NST_128x160 2
#endif
#ifndef UR_NST_128x64
#define UR_NST_128x64 2
#endif
#ifndef UR_NST_64x64
#define UR_NST_64x64 2
#endif

namespace urk {
UR_LAUNCHER(g1_128x128, Gemm<128, 128, 2, 2, UR_NST_128x128, true>)
UR_LAUNCHER(g1_128x160, Gemm<128, 160, 4, 1, UR_NST_128x160, true>)
UR_LAUNCHER(g1_128x64, Gemm<128, 64, 2, 2, UR_NST_128x64, true>)
UR_LAUNCHER(g1_64x64, Gemm<64, 64, 2, 2, UR_NST_64x64, true>)
// deeper rings where the round-5 sweep (profiles/r5_wreg_ab.txt) found them: 64 x 64 / 4 stages for grids of <= 256 workgroups (the 8x8
// level: less than one workgroup per CU IS latency-bound: 512 x 1280 x 1280 12.9 -> 9.1 us), 128 x 64 / 3 stages unsplit for the long-K
// 16x16-level GEMMs (2048 x 1280 x 2560 25.9 -> 23.3 us, x 5120 49.1 -> 43.7 us against split-K + reduce)
UR_LAUNCHER(g1_64x64_deep, Gemm<64, 64, 2, 2, 4, true>)
UR_LAUNCHER(g1_128x64_deep, Gemm<128, 64, 2, 2, 3, true>)
}  // namespace urk
