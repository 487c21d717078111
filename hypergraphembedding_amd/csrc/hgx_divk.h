// The trainer step's divisions by the neighbour count, x / (float)K for a
// compile-time K, in a header host code can include: the device kernels and
// the exhaustive host check (tests/native/div_const_check.cpp) run the same
// text.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HGX_DIVK_HD __host__ __device__ __forceinline__
#else
#define HGX_DIVK_HD inline
#endif

// x / (float)K, correctly rounded, without the IEEE division sequence (on
// gfx950 a dependent chain of about twelve instructions with a
// transcendental): q = x r with r = RN(1 / K), the exact residual
// e = x - K q by one fma, and the correction q + e r by another. Without a
// residual the quotient stands as it is: e == 0 (the correction would turn
// -0 into +0) and e NaN (an infinite x: inf - inf; q is the infinity the
// division returns). Used only for the K that tests/test_div_const.py proves equal
// to x / (float)K for every float bit pattern (denormals, infinities and
// NaNs included; built with contraction off).
template <int K>
HGX_DIVK_HD float div_const(float x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  constexpr float r = 1.0f / (float)K;
  const float q = x * r;
  const float e = __builtin_fmaf(-(float)K, q, x);
  const float c = __builtin_fmaf(e, r, q);
  return __builtin_fabsf(e) > 0.f ? c : q;
}
