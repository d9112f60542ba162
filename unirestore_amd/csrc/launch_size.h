// Block count of a 1-D launch, computed and checked on the host in 64 bits.  No HIP in here: common.h includes it for every
// kernel file, and tests/launch_size_main.cpp compiles it alone with the host compiler under UBSan / ASan.
//
// Why a limit below 2^31: the 1-D kernels form `const int i = blockIdx.x * B + threadIdx.x` (an unsigned product narrowed to int)
// and leave with `if (i >= total) return;`.  The threads of the last block that lie past `total` must still have an index that
// fits an int, or it turns negative and passes that test: with B <= 256 and total < 2^31 - 256 the whole last block stays below
// 2^31.  (`(total + B - 1) / B` in int arithmetic overflows for total > INT_MAX - B + 1 as well: here it is done in long long.)
#pragma once
#include <string>

#include "../../include/unirestore_hip.h"

namespace ur {
int fail(int code, const std::string& msg);

constexpr long long GRID_1D_LIMIT = (1ll << 31) - 256;      // work items of one 1-D launch: count < GRID_1D_LIMIT
constexpr int GRID_1D_MAX_BLOCK = 256;                      // the margin above holds for blocks of at most this many threads

// *blocks = ceil(count / per_block) and 0, or UR_E_INVALID (message: `who`, the entry point) for a count outside [1, 2^31 - 256)
// or a per_block outside [1, 256]; *blocks is 0 then.
inline int grid_1d(const char* who, long long count, int per_block, unsigned* blocks) {
  *blocks = 0;
  if (per_block < 1 || per_block > GRID_1D_MAX_BLOCK)
    return fail(UR_E_INVALID, std::string(who) + ": grid_1d: per_block must be in [1, 256], got " + std::to_string(per_block));
  if (count < 1 || count >= GRID_1D_LIMIT)
    return fail(UR_E_INVALID, std::string(who) + ": a launch of " + std::to_string(count) + " work items: the count must be in [1, 2^31 - 256)");
  *blocks = (unsigned)((count + per_block - 1) / per_block);
  return 0;
}
}  // namespace ur

// `unsigned var` = the block count of `count` work items in blocks of `per_block`; returns UR_E_INVALID from the calling entry
// point (named in the message) when the count is out of range.
#define UR_GRID_1D(var, count, per_block)                                          \
  unsigned var = 0;                                                                \
  do {                                                                             \
    if (int ur_rc_ = ur::grid_1d(__func__, (count), (per_block), &var)) return ur_rc_; \
  } while (0)
