"""Host check of csrc/resize.hip: the three kernels and the launch function's pass logic compiled as plain C++ for the CPU, every launch a
loop over its threads, run under the address and undefined-behaviour sanitizers on exact-size heap buffers against the numpy
restatement of tests/resize_reference.py, on the case list of tests/resize_cases.py in both modes and all image kinds.

  python tools/resize_host_check.py [--cxx clang++] [--keep DIR]

The kernels have no barriers and no cross-thread traffic, so running the threads one after another computes what the launch does.
Exit status 0 when every output byte is equal; the sanitizers abort on any access outside a buffer."""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests")]

PRE = r'''
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <vector>
struct D3 { unsigned x, y, z; };
static D3 threadIdx{0,0,0}, blockIdx{0,0,0};
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
using std::min; using std::max;
namespace {
'''

POST = r'''}  // namespace
template <class F> static void launch(long long threads, F f) {
  for (long long b = 0; b < (threads + 255) / 256; ++b) for (unsigned t = 0; t < 256; ++t) { blockIdx.x = (unsigned)b; threadIdx.x = t; f(); }
}
static std::vector<int32_t> read_i32(FILE* f, size_t n) { std::vector<int32_t> v(n); if (fread(v.data(), 4, n, f) != n) exit(3); return v; }
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb");
  int bad = 0, cases = 0;
  int32_t h[9];
  while (fread(h, 4, 9, f) == 9) {
    const int N = h[0], H = h[1], W = h[2], oh = h[3], ow = h[4], xK = h[5], xp = h[6], yK = h[7], yp = h[8];
    // exact-size heap copies of every table and image: the address sanitizer sees any access outside them
    std::vector<int32_t> xb = read_i32(f, 2 * ow), xw = read_i32(f, (size_t)ow * xK), yb = read_i32(f, 2 * oh), yw = read_i32(f, (size_t)oh * yK);
    const size_t in_b = (size_t)N * H * W * 3, mid_b = (size_t)N * H * ow * 3, out_b = (size_t)N * oh * ow * 3;
    uint8_t* x = (uint8_t*)malloc(in_b); uint8_t* mid = (uint8_t*)malloc(mid_b); uint8_t* out = (uint8_t*)malloc(out_b); uint8_t* want = (uint8_t*)malloc(out_b);
    if (fread(x, 1, in_b, f) != in_b || fread(want, 1, out_b, f) != out_b) return 3;
    memset(mid, 0xA5, mid_b); memset(out, 0xA5, out_b);
    const bool along_w = ow != W, along_h = oh != H;          // the pass logic of ur_resize_u8
    if (!along_w && !along_h) launch((long long)in_b, [&] { resize_copy_kernel(x, out, (long long)in_b); });
    else {
      const uint8_t* src = x;
      if (along_w) {
        uint8_t* dst = along_h ? mid : out;
        launch((long long)N * H * ow, [&] { resize_width_kernel(x, dst, (long long)N * H * ow, W, ow, xb.data(), xw.data(), xK, xp); });
        src = dst;
      }
      if (along_h) launch((long long)out_b, [&] { resize_height_kernel(src, out, (long long)out_b, H, oh, ow * 3, yb.data(), yw.data(), yK, yp); });
    }
    const int diff = memcmp(out, want, out_b) != 0;
    if (diff) printf("MISMATCH N%d %dx%d -> %dx%d K %d/%d p %d/%d\n", N, H, W, oh, ow, xK, yK, xp, yp);
    bad += diff; ++cases;
    // a table row that points outside the image is read as empty: no access outside x (the sanitizer is the check)
    xb[0] = -1; xb[3] = xK + 1; yb[0] = H; yb[2] = H - 1; yb[3] = 2;
    if (along_w) launch((long long)N * H * ow, [&] { resize_width_kernel(x, mid, (long long)N * H * ow, W, ow, xb.data(), xw.data(), xK, xp); });
    if (along_h && !along_w) launch((long long)out_b, [&] { resize_height_kernel(x, out, (long long)out_b, H, oh, ow * 3, yb.data(), yw.data(), yK, yp); });
    free(x); free(mid); free(out); free(want);
  }
  printf("%d cases, %d differ from the restatement\n", cases, bad);
  return bad != 0 || cases == 0;
}
'''


def main():
    import resize_cases as cases
    import resize_reference as ref
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=None)
    ap.add_argument("--keep", default=None, help="write host_resize.cpp, the case file and the program here instead of a temporary folder")
    a = ap.parse_args()
    cxx = a.cxx or next((c for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")) if c and os.path.exists(c)), None)
    if cxx is None:
        raise SystemExit("no C++ compiler found (--cxx)")
    src = open(os.path.join(ROOT, "unirestore_amd", "csrc", "resize.hip")).read()
    body = src.split("namespace {", 1)[1].split("inline unsigned blocks_of", 1)[0]
    out = a.keep or tempfile.mkdtemp(prefix="resize_host_")
    os.makedirs(out, exist_ok=True)
    cpp, exe, dat = os.path.join(out, "host_resize.cpp"), os.path.join(out, "host_resize"), os.path.join(out, "cases.bin")
    with open(cpp, "w") as f:
        f.write(PRE + body + POST)
    with open(dat, "wb") as f:
        for mode in cases.MODES:
            for shape, size in cases.CASES:
                xb, xw, xk, xp = ref.axis_tables(shape[2], size[1], mode)
                yb, yw, yk, yp = ref.axis_tables(shape[1], size[0], mode)
                for kind in cases.KINDS:
                    x = cases.images(shape, kind)
                    f.write(np.array([*shape, *size, xk, xp, yk, yp], dtype=np.int32).tobytes())
                    for t in (xb, xw, yb, yw):
                        f.write(np.ascontiguousarray(t, dtype=np.int32).tobytes())
                    f.write(x.tobytes())
                    f.write(ref.resize(x, size, mode).tobytes())
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, cpp], check=True)
    rc = subprocess.run([exe, dat]).returncode
    if not a.keep:
        shutil.rmtree(out, ignore_errors=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
