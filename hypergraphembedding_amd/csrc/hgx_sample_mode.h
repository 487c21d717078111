// The rejection sampler's automatic choice between its two 3-hop proposals
// (csrc/hgx_sample.hip, reject_rows), in a header host code can include: the
// device kernel and the host check (tests/native/sample_mode_check.cpp) run
// the same text.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HGX_SMODE_HD __host__ __device__ __forceinline__
#else
#define HGX_SMODE_HD inline
#endif

// A 3-hop row with W paths over ncols columns proposes uniform columns
// (acceptance |row| / ncols) instead of uniform paths (|row| / W) when
// W >= ncols * 2^shift, shift in [-10, 10] (sample_mode3_shift). For a
// negative shift W is not scaled up (W << -shift leaves 64 bits from
// W = 2^53 on): W 2^s >= ncols  <=>  W >= ceil(ncols / 2^s) for integers, so
// ncols is scaled down, rounding up. ncols < 2^31, so neither side
// overflows for any W >= 0.
HGX_SMODE_HD bool sample_mode3_uniform(long long W, int ncols, int shift) {
  if (shift >= 0) return W >= ((long long)ncols << shift);
  const int s = -shift;
  return W >= (((long long)ncols + ((1ll << s) - 1)) >> s);
}
