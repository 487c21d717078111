// Exhaustive host check of the trainer step's float -> 2^44 fixed-point
// conversion in its add-constant form (to_fix_magic of csrc/hgx_fix.h, the
// text the device kernels compile): every float bit pattern with
// |v| < kFixLimit, denormals and -0 included, against
// llrint((double)v * 0x1p44) under round-to-nearest. Reports the first
// difference and exits non-zero. At most 16 threads. Built and run by
// tests/test_to_fix.py (-O2 -fopenmp -fsanitize=undefined).
#include <atomic>
#include <cfenv>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include <omp.h>

#include "hgx_fix.h"

int main() {
  static_assert(kFixScale == 0x1p44, "the scale the reference multiplies by");
  uint32_t lim;
  const float limit = kFixLimit;
  memcpy(&lim, &limit, 4);  // magnitudes below this bit pattern are in range
  const int nt = omp_get_max_threads() < 16 ? omp_get_max_threads() : 16;
  std::atomic<int> bad{0};
  long long checked = 0;
#pragma omp parallel num_threads(nt) reduction(+ : checked)
  {
    fesetround(FE_TONEAREST);
#pragma omp for schedule(static)
    for (int64_t m = 0; m < (int64_t)lim; m++) {
      if (bad.load(std::memory_order_relaxed)) continue;
      for (uint32_t sign = 0; sign < 2; sign++) {
        const uint32_t bits = (uint32_t)m | (sign << 31);
        float v;
        memcpy(&v, &bits, 4);
        const long long want = llrint((double)v * 0x1p44);
        const long long got = (long long)to_fix_magic(v);
        checked++;
        if (got != want && !bad.exchange(1))
          fprintf(stderr, "to_fix_magic(%a) [0x%08x] = %lld, llrint gives %lld\n", (double)v, bits, got,
                  want);
      }
    }
  }
  if (bad) return 1;
  printf("%lld patterns, %d threads: identical\n", checked, nt);
  return checked == 2 * (long long)lim ? 0 : 2;
}
