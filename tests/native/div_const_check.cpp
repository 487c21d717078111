// Exhaustive host check of the trainer step's division by a constant
// (div_const<K> of csrc/hgx_divk.h, the text the device kernels compile):
// every one of the 2^32 float bit patterns, denormals, infinities and NaNs
// included, against x / (float)K under round-to-nearest, for every K given
// on the command line (the K that have a step kernel). Equal bits, or NaN on
// both sides, count as equal. Reports the first difference of each K and
// exits non-zero. At most 16 threads. Built and run by
// tests/test_div_const.py (-O2 -ffp-contract=off -fopenmp).
#include <atomic>
#include <cfenv>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <omp.h>

#include "hgx_divk.h"

template <int K>
static long long check(int nt, int &bad_out) {
  std::atomic<int> bad{0};
  long long checked = 0;
#pragma omp parallel num_threads(nt) reduction(+ : checked)
  {
    fesetround(FE_TONEAREST);
#pragma omp for schedule(static)
    for (int64_t hi = 0; hi < (1 << 16); hi++) {
      if (bad.load(std::memory_order_relaxed)) continue;
      for (uint32_t lo = 0; lo < (1u << 16); lo++) {
        const uint32_t bits = ((uint32_t)hi << 16) | lo;
        float x;
        memcpy(&x, &bits, 4);
        volatile float kf = (float)K;  // (a division the compiler cannot rewrite)
        const float want = x / kf;
        const float got = div_const<K>(x);
        uint32_t wb, gb;
        memcpy(&wb, &want, 4);
        memcpy(&gb, &got, 4);
        checked++;
        if (wb != gb && !(std::isnan(want) && std::isnan(got)) && !bad.exchange(1))
          fprintf(stderr, "div_const<%d>(%a) [0x%08x] = %a [0x%08x], the division gives %a [0x%08x]\n",
                  K, (double)x, bits, (double)got, gb, (double)want, wb);
      }
    }
  }
  bad_out |= bad.load();
  return checked;
}

int main(int argc, char **argv) {
  const int nt = omp_get_max_threads() < 16 ? omp_get_max_threads() : 16;
  int bad = 0;
  for (int i = 1; i < argc; i++) {
    const int K = atoi(argv[i]);
    long long n = 0;
    if (K == 5) n = check<5>(nt, bad);
    else {
      fprintf(stderr, "no step kernel for K = %d\n", K);
      return 2;
    }
    if (!bad && n != (1ll << 32)) return 2;
    printf("K = %d: %lld patterns, %d threads: %s\n", K, n, nt, bad ? "DIFFERENT" : "identical");
  }
  return bad ? 1 : 0;
}
