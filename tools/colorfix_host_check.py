"""Host check of csrc/colorfix.hip's indexing: the two wavelet kernels and the AdaIN apply kernel compiled as plain C++ for the CPU
and run under the address and undefined-behaviour sanitizers against a whole-canvas loop in the same arithmetic order.

  python tools/colorfix_host_check.py [--cxx clang++] [--keep DIR]

Every phase of these kernels is a `for (e = threadIdx.x; e < n; e += 256)` loop between barriers, so ONE thread with stride 1 runs a
phase's elements in sequence and a barrier is a no-op: the same values as the parallel launch, provided the phases are race-free
(that is argued in the kernel's comments, not checked here).  Exact-size heap buffers and the static LDS arrays give the sanitizer
every bound.  The statistics and finalize kernels (wave shuffles, phases keyed on the thread index) are left to the GPU tests.
Shapes: the case table of tests/colorfix_cases.py and two long thin ones, each with the vector and the scalar access path.
Exit status 0 when every output is bit-equal (wavelet) / within 1e-6 (apply) and the padding channels are zeros.
"""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PRE = r'''
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <algorithm>
#include <vector>
struct D3 { unsigned x, y, z; };
static D3 threadIdx{0,0,0}, blockIdx{0,0,0};
#define __global__
#define __device__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(x)
#define __restrict__
inline void __syncthreads() {}
struct float4 { float x, y, z, w; };
inline float4 make_float4(float a, float b, float c, float d) { return float4{a,b,c,d}; }
struct uint2 { uint32_t x, y; };
using std::min; using std::max;
inline float bits2f(uint32_t u) { float f; memcpy(&f,&u,4); return f; }
template <bool F16> struct Act {
  static float lo(uint32_t w) { return bits2f(w << 16); }
  static float hi(uint32_t w) { return bits2f(w & 0xffff0000u); }
  static float one(uint16_t v) { return bits2f(((uint32_t)v) << 16); }
};

'''

POST = r'''}  // namespace
static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
int run(int N, int src_n, int H, int W, int ld_c, int ld_s, int vec_c, int vec_s) {
  size_t P = (size_t)H * W;
  // exact-size heap buffers: the address sanitizer sees any access outside them
  float* c = (float*)malloc(N * P * ld_c * 4); float* out = (float*)malloc(N * P * ld_c * 4); float* out2 = (float*)malloc(N * P * ld_c * 4);
  uint16_t* s = (uint16_t*)malloc(src_n * P * ld_s * 2);
  srand(N * 7 + H * 131 + W);
  for (size_t i = 0; i < N * P * ld_c; ++i) { c[i] = (i % ld_c) < 3 ? (rand() / (float)RAND_MAX) * 2 - 1 : NAN; out[i] = NAN; out2[i] = NAN; }
  for (size_t i = 0; i < src_n * P * ld_s; ++i) { float v = (rand() / (float)RAND_MAX) * 2 - 1; uint32_t u; memcpy(&u, &v, 4); s[i] = (i % ld_s) < 3 ? (uint16_t)(u >> 16) : 0x7fc0; }
  const int tx = (W + CF_VC - 1) / CF_VC, ty = (H + CF_VR - 1) / CF_VR, hy = (H + CF_HR - 1) / CF_HR;
  for (unsigned b = 0; b < (unsigned)(N * tx * ty); ++b) { blockIdx.x = b; cf_wavelet_cols_kernel<false>(c, ld_c, s, ld_s, out, src_n, H, W, tx, ty, vec_c, vec_s); }
  for (unsigned b = 0; b < (unsigned)(N * hy); ++b) { blockIdx.x = b; cf_wavelet_rows_kernel(c, ld_c, out, H, W, hy, vec_c); }
  // whole-canvas reference in the same arithmetic order
  int bad = 0;
  std::vector<float> v(P), t(P);
  for (int n = 0; n < N; ++n) for (int k = 0; k < 3; ++k) {
    for (size_t p = 0; p < P; ++p) v[p] = Act<false>::one(s[((size_t)(n % src_n) * P + p) * ld_s + k]) - c[((size_t)n * P + p) * ld_c + k];
    for (int r = 1; r <= 16; r <<= 1) { for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) t[(size_t)y*W+x] = 0.25f * (v[(size_t)clampi(y-r,0,H-1)*W+x] + v[(size_t)clampi(y+r,0,H-1)*W+x]) + 0.5f * v[(size_t)y*W+x]; v.swap(t); }
    for (int r = 1; r <= 16; r <<= 1) { for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) t[(size_t)y*W+x] = 0.25f * (v[(size_t)y*W+clampi(x-r,0,W-1)] + v[(size_t)y*W+clampi(x+r,0,W-1)]) + 0.5f * v[(size_t)y*W+x]; v.swap(t); }
    for (size_t p = 0; p < P; ++p) { float want = c[((size_t)n * P + p) * ld_c + k] + v[p], got = out[((size_t)n * P + p) * ld_c + k]; if (memcmp(&want, &got, 4)) { if (bad < 5) printf("  mismatch n%d k%d p%zu want %g got %g\n", n, k, p, want, got); ++bad; } }
  }
  for (size_t i = 0; i < N * P * ld_c; ++i) if ((i % ld_c) >= 3 && out[i] != 0.f) ++bad;
  // adain apply
  std::vector<float> ab(N * 6); for (auto& x : ab) x = (rand() / (float)RAND_MAX) * 2 - 1;
  long long blocks = ((long long)P + 255) / 256;
  for (unsigned b = 0; b < (unsigned)(N * blocks); ++b) for (unsigned th = 0; th < 256; ++th) { blockIdx.x = b; threadIdx.x = th; cf_adain_apply_kernel(c, ld_c, ab.data(), out2, (long long)P, (int)blocks, vec_c); }
  threadIdx.x = 0;
  for (int n = 0; n < N; ++n) for (size_t p = 0; p < P; ++p) for (int k = 0; k < ld_c; ++k) { float got = out2[((size_t)n*P+p)*ld_c+k]; float want = k < 3 ? ab[n*6+2*k] * c[((size_t)n*P+p)*ld_c+k] + ab[n*6+2*k+1] : 0.f; if (!(fabsf(got - want) <= 1e-6f)) ++bad; }
  printf("N%d src%d %dx%d ld %d/%d vec %d/%d: %s (%d)\n", N, src_n, H, W, ld_c, ld_s, vec_c, vec_s, bad ? "MISMATCH" : "ok", bad);
  free(c); free(out); free(out2); free(s);
  return bad;
}
int main() {
  int bad = 0;
  int sh[][6] = {{1,1,1,1,8,8},{1,1,1,40,8,8},{2,2,3,5,8,8},{2,1,17,33,4,8},{3,3,31,32,8,16},{1,1,63,64,3,8},{1,1,170,200,8,8},{2,1,199,170,4,16},{4,2,20,24,8,8},{1,1,70,300,8,8},{1,1,300,7,5,3}};
  for (auto& q : sh) { bad += run(q[0],q[1],q[2],q[3],q[4],q[5], q[4] % 4 == 0, q[5] % 4 == 0); bad += run(q[0],q[1],q[2],q[3],q[4],q[5], 0, 0); }
  return bad != 0;
}
'''


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=None)
    ap.add_argument("--keep", default=None, help="write host_cf.cpp and the program here instead of a temporary folder")
    a = ap.parse_args()
    cxx = a.cxx or next((c for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")) if c and os.path.exists(c)), None)
    if cxx is None:
        raise SystemExit("no C++ compiler found (--cxx)")
    src = open(os.path.join(ROOT, "unirestore_amd", "csrc", "colorfix.hip")).read()
    body = src.split("#include <climits>")[1].split("inline bool aligned")[0]
    body = body.replace("e += 256", "e += 1").replace("p += 256", "p += 1")
    body = body[:body.index("// pass 1: fp64 (sum, sum of squares)")] + body[body.index("// pass 3: out = a * c + b"):]
    out = a.keep or tempfile.mkdtemp(prefix="colorfix_host_")
    os.makedirs(out, exist_ok=True)
    cpp, exe = os.path.join(out, "host_cf.cpp"), os.path.join(out, "host_cf")
    with open(cpp, "w") as f:
        f.write(PRE + body + POST)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-o", exe, cpp], check=True)
    rc = subprocess.run([exe]).returncode
    if not a.keep:
        shutil.rmtree(out, ignore_errors=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
