// Host check of the rejection sampler's automatic 3-hop mode choice
// (sample_mode3_uniform of csrc/hgx_sample_mode.h, the text the device
// kernel compiles) against 128-bit integer arithmetic: uniform columns iff
// W >= ncols * 2^shift over the rationals.
// For a few thousand ncols up to 2^31 - 1 and every shift in [-10, 10] it
// checks W at the threshold and at +-1, W = 0, 1, every power of two up to
// 2^62 with its neighbours, and pseudo-random W below 2^62. It also checks
// that the comparison the kernel used before (W << -shift for a negative
// shift) gave the same answer wherever that shift did not overflow. Reports
// the first difference and exits non-zero. Built and run by
// tests/test_sample_mode.py (once more with -fsanitize=undefined).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "hgx_sample_mode.h"

typedef __int128 i128;

static bool want(long long W, int ncols, int shift) {
  // W >= ncols * 2^shift  <=>  W * 2^max(-shift, 0) >= ncols * 2^max(shift, 0)
  const i128 l = (i128)W << (shift < 0 ? -shift : 0);
  const i128 r = (i128)ncols << (shift > 0 ? shift : 0);
  return l >= r;
}

static uint64_t mix(uint64_t z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

int main() {
  std::vector<int> ncols;
  for (int n = 1; n <= 2050; n++) ncols.push_back(n);
  for (int b = 11; b <= 31; b++)
    for (int d = -3; d <= 3; d++) {
      const long long n = (1ll << b) + d;
      if (n > 0 && n <= 0x7fffffffll) ncols.push_back((int)n);
    }
  for (int n : {393216, 393217, 1000003, 123456789, 2147483646, 2147483647}) ncols.push_back(n);
  for (int i = 0; i < 2000; i++) ncols.push_back((int)(mix(i) % 0x7fffffffull) + 1);
  long long checked = 0, old_same = 0;
  for (int nc : ncols) {
    for (int shift = -10; shift <= 10; shift++) {
      std::vector<long long> ws = {0, 1, 2, (1ll << 62) - 1, 1ll << 62};
      // threshold: the least W with W >= ncols * 2^shift
      const i128 num = (i128)nc << (shift > 0 ? shift : 0);
      const i128 den = (i128)1 << (shift < 0 ? -shift : 0);
      const long long thr = (long long)((num + den - 1) / den);
      for (long long d = -2; d <= 2; d++)
        if (thr + d >= 0) ws.push_back(thr + d);
      for (int b = 1; b <= 62; b++)
        for (long long d = -1; d <= 1; d++)
          if ((1ll << b) + d <= (1ll << 62)) ws.push_back((1ll << b) + d);
      for (int i = 0; i < 16; i++)
        ws.push_back((long long)(mix(((uint64_t)nc << 8) ^ (uint64_t)(shift + 16) ^ ((uint64_t)i << 40)) >>
                                 (2 + (i * 4) % 60)));
      for (long long W : ws) {
        const bool w = want(W, nc, shift);
        const bool g = sample_mode3_uniform(W, nc, shift);
        checked++;
        if (g != w) {
          fprintf(stderr, "sample_mode3_uniform(%lld, %d, %d) = %d, exact %d\n", W, nc, shift,
                  (int)g, (int)w);
          return 1;
        }
        // the comparison this header replaced, where it was defined
        if (shift >= 0 || W < (1ll << (62 + shift))) {
          const bool old = shift >= 0 ? W >= ((long long)nc << shift)
                                      : (W << -shift) >= (long long)nc;
          old_same++;
          if (old != g) {
            fprintf(stderr, "former comparison differs at (%lld, %d, %d): %d vs %d\n", W, nc,
                    shift, (int)old, (int)g);
            return 1;
          }
        }
      }
    }
  }
  printf("%zu ncols, 21 shifts, %lld comparisons identical to 128-bit arithmetic, %lld to the "
         "former comparison\n",
         ncols.size(), checked, old_same);
  return 0;
}
