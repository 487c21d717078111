// np.linalg.norm of the float32 vector a - b, bit for bit, on the device.
//
// `norm` is np.linalg.norm: sqrt(x.dot(x)), OpenBLAS sdot through numpy's
// FLOAT_dot. The fixtures (tests/golden/make_golden_weights.py) were made
// with numpy's OpenBLAS 0.3.29, SkylakeX kernel; norm32 restates its
// arithmetic (probed against numpy on 3,000 random vectors of 10-130
// elements, no difference): the first k & ~31 elements in 4 accumulators x 8
// lanes (fused multiply-add; blocks of 64 first go through 4 x 16 lanes
// folded lane l + l+8), accumulators summed ((a0 + a1) + a2) + a3, then
// lanes l + l+4, then (h0 + h1) + (h2 + h3); the rest added in DOUBLE as
// float products; the float of that, float sqrt. Below k = 32 only the
// double tail runs.
//
// Used by hgx_weights.hip (hg2v_weighting's distances) and, from k = 32 on,
// by hgx_hobe.hip (the HOBE weights).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace hgx {

__device__ inline float norm32(const float *__restrict__ a,
                               const float *__restrict__ b, int k) {
// No implicit contraction inside: the explicit fmas are the reference's,
// and a float product added to a double must not become a double fma (hipcc
// contracts by default).
#pragma clang fp contract(off)
  const int n1 = k & ~31, n64 = n1 & ~63;
  int i = 0;
  float tot = 0.f;
  if (n1) {
    float acc[32];
#pragma unroll
    for (int t = 0; t < 32; t++) acc[t] = 0.f;
    if (n64) {
      float a5[64];
#pragma unroll
      for (int t = 0; t < 64; t++) a5[t] = 0.f;
      for (; i < n64; i += 64) {
#pragma unroll
        for (int t = 0; t < 64; t++) {
          const float d = a[i + t] - b[i + t];
          a5[t] = __fmaf_rn(d, d, a5[t]);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int l = 0; l < 8; l++)
          acc[j * 8 + l] = a5[j * 16 + l] + a5[j * 16 + l + 8];
    }
    for (; i < n1; i += 32) {
#pragma unroll
      for (int t = 0; t < 32; t++) {
        const float d = a[i + t] - b[i + t];
        acc[t] = __fmaf_rn(d, d, acc[t]);
      }
    }
    float s[8];
#pragma unroll
    for (int l = 0; l < 8; l++)
      s[l] = ((acc[l] + acc[8 + l]) + acc[16 + l]) + acc[24 + l];
    float h[4];
#pragma unroll
    for (int l = 0; l < 4; l++) h[l] = s[l] + s[l + 4];
    tot = (h[0] + h[1]) + (h[2] + h[3]);
  }
  double dot = tot;
  for (; i < k; i++) {
    const float d = a[i] - b[i];
    const float p = d * d;
    dot = dot + (double)p;
  }
  // correctly rounded float sqrt (v_sqrt_f32 is not): through double
  return (float)sqrt((double)(float)dot);
}

}  // namespace hgx
