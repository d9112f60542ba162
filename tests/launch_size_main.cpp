// Stand-alone host check of ur::grid_1d (unirestore_amd/csrc/launch_size.h): no HIP, no Python.  tests/test_scoring_large_cpu.py
// compiles it with the host compiler under -fsanitize=undefined,address and runs it; every expected value below is a literal
// worked out by hand in arbitrary precision (2^31 = 2147483648, 2^32 = 4294967296).
#include <cstdio>
#include <string>

#include "../unirestore_amd/csrc/launch_size.h"

static int g_code = 0;
static std::string g_msg;
namespace ur {
int fail(int code, const std::string& msg) {
  g_code = code;
  g_msg = msg;
  return code;
}
}  // namespace ur

struct Row {
  long long count;
  int per_block;
  bool accepted;
  unsigned blocks;      // when accepted
};

int main() {
  const Row rows[] = {
      {1LL, 256, true, 1u},
      {255LL, 256, true, 1u},
      {256LL, 256, true, 1u},
      {257LL, 256, true, 2u},
      {2147483391LL, 256, true, 8388607u},      // 2^31 - 257: the largest accepted count; 8388607 * 256 = 2147483392 = 2^31 - 256
      {2147483392LL, 256, false, 0u},           // 2^31 - 256: the limit itself
      {2147483647LL, 256, false, 0u},           // 2^31 - 1: `count + 255` overflows an int
      {4294967296LL, 256, false, 0u},           // 2^32: truncates to 0 in 32 bits
      {0LL, 256, false, 0u},
      {-1LL, 256, false, 0u},
      {1LL, 64, true, 1u},
      {65LL, 64, true, 2u},
      {2147483391LL, 64, true, 33554428u},      // 33554428 * 64 = 2147483392
      {2147483391LL, 4, true, 536870848u},      // 536870848 * 4 = 2147483392
      {2147483391LL, 1, true, 2147483391u},
      {100LL, 0, false, 0u},
      {100LL, 257, false, 0u},                  // the margin of 256 covers blocks of at most 256 threads
  };
  int bad = 0;
  for (const Row& r : rows) {
    g_code = 0;
    g_msg.clear();
    unsigned blocks = 12345u;
    const int rc = ur::grid_1d("ur_some_entry_point", r.count, r.per_block, &blocks);
    bool ok;
    if (r.accepted) {
      ok = rc == 0 && blocks == r.blocks && g_code == 0;
      // the whole last block stays inside an int: blocks * per_block <= 2^31 - 256 + (per_block - 1) < 2^31
      ok = ok && (unsigned long long)blocks * (unsigned long long)r.per_block <= 2147483647ULL;
    } else {
      ok = rc == UR_E_INVALID && g_code == UR_E_INVALID && blocks == 0u && g_msg.find("ur_some_entry_point") == 0;
    }
    std::printf("%s count %lld per_block %d -> rc %d blocks %u %s\n", ok ? "ok  " : "FAIL", r.count, r.per_block, rc, blocks, g_msg.c_str());
    bad += !ok;
  }
  if (ur::GRID_1D_LIMIT != 2147483392LL) {
    std::printf("FAIL GRID_1D_LIMIT %lld\n", ur::GRID_1D_LIMIT);
    ++bad;
  }
  std::printf("%s\n", bad ? "FAILED" : "PASSED");
  return bad ? 1 : 0;
}
