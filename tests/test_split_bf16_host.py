"""CPU test of the host-visible parts of csrc/lgx_split_bf16.h (the pre-split operand image) and
csrc/lgx_launch.h (the persistent grid): a stand-alone C++ program with its own main, compiled with
the host compiler ($CXX, else c++) under the address and undefined-behaviour sanitizers, and run.
Nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "legged_gym_amd", "csrc")

PROGRAM = r"""
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "lgx_launch.h"
#include "lgx_split_bf16.h"

static int fails = 0;
#define CHECK(cond, ...) \
  do { if (!(cond)) { if (++fails <= 20) { std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

int main() {
  // the image's sizes, by their names
  CHECK(LGX_X3_PLANE == 128 * 32 && LGX_X3_BLOCK == 3 * LGX_X3_PLANE && LGX_X3_UNIT == 96, "named sizes");
  for (int N : {128, 256})
    for (int K : {32, 40, 64, 235}) {
      const int kb = (K + 31) / 32;
      const int64_t range = (int64_t)N * kb * 96;
      const int64_t elems = x3_image_elems(N, K);
      CHECK(elems == (int64_t)N * kb * LGX_X3_UNIT && elems == range, "N %d K %d: elems %lld", N, K, (long long)elems);
      CHECK(elems == (int64_t)(N / LGX_X3_BN) * kb * LGX_X3_BLOCK, "N %d K %d: elems in blocks", N, K);
      std::vector<uint8_t> hit(range, 0);
      int64_t asked = 0;
      for (int n = 0; n < N; ++n)
        for (int k = 0; k < K; ++k)
          for (int limb = 0; limb < 3; ++limb) {
            const int64_t o = x3_limb_off(n, k, limb, kb);
            CHECK(o >= 0 && o < range && o < elems, "N %d K %d: (%d, %d, %d) -> %lld out of range", N, K, n, k, limb,
                  (long long)o);
            if (o < 0 || o >= range) continue;
            CHECK(!hit[o], "N %d K %d: (%d, %d, %d) collides at %lld", N, K, n, k, limb, (long long)o);
            hit[o] = 1;
            ++asked;
            CHECK(o == x3_limb_off(n, k, 0, kb) + (int64_t)limb * LGX_X3_PLANE, "N %d K %d: (%d, %d) limb %d plane", N,
                  K, n, k, limb);
          }
      // onto: with the padding positions k in [K, 32 kb) the offsets fill the range exactly, and no
      // padding position lands on one that was asked for
      for (int n = 0; n < N; ++n)
        for (int k = K; k < 32 * kb; ++k)
          for (int limb = 0; limb < 3; ++limb) {
            const int64_t o = x3_limb_off(n, k, limb, kb);
            CHECK(o >= 0 && o < range && !hit[o], "N %d K %d: padding (%d, %d, %d) at %lld", N, K, n, k, limb,
                  (long long)o);
            if (o >= 0 && o < range) hit[o] = 2;
          }
      CHECK(asked == (int64_t)N * K * 3, "N %d K %d: asked %lld", N, K, (long long)asked);
      CHECK(std::count(hit.begin(), hit.end(), 0) == 0, "N %d K %d: positions never written", N, K);
    }
  // the persistent grid against the expression it replaced, written out
  for (int64_t tiles = 1; tiles <= 4096; ++tiles)
    for (int cus : {8, 64, 256, 304})
      for (int k : {1, 2}) {
        const int64_t ref = 8 * std::min<int64_t>((tiles + 7) / 8, std::max(1, k * cus / 8));
        const int64_t got = lgx_xcd_grid(tiles, cus, k);
        CHECK(got == ref && got > 0 && got % 8 == 0, "grid(%lld, %d, %d) = %lld, expected %lld", (long long)tiles, cus, k,
              (long long)got, (long long)ref);
      }
  std::printf("%s\n", fails ? "FAILED" : "ok");
  return fails ? 1 : 0;
}
"""


def test_limb_image_is_a_bijection_and_the_grid_is_the_old_expression(tmp_path):
    src, exe = tmp_path / "split_bf16_host.cpp", tmp_path / "split_bf16_host"
    src.write_text(PROGRAM)
    cxx = os.environ.get("CXX") or "c++"
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), str(src)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr
