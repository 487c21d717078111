// The trainer step's 2^44 fixed point (deferred-row and padding-row gradient
// sums, see hgx_train_step.h), in a header host code can include: the device
// kernels and the exhaustive host check (tests/native/to_fix_check.cpp) run
// the same text.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HGX_FIX_HD __host__ __device__ __forceinline__
#else
#define HGX_FIX_HD inline
#endif

// 2^44 units, |one added value| < kFixLimit; at most 2^13 adds per entry and
// batch keep the sum below 2^63. A value outside the range (a diverged run, or
// NaN) raises the step's overflow flag and hgx_train fails with HGX_ENUMERIC.
constexpr double kFixScale = 17592186044416.0;  // 2^44
constexpr double kFixInv = 1.0 / 17592186044416.0;
constexpr float kFixLimit = 32.f;

// Two texts of the same conversion, to_fix_magic and to_fix_rn (identical
// integers for every |v| < kFixLimit: tests/test_to_fix.py), picked per row
// width by to_fix<VW>. HGX_TRAIN_FIXMAGIC: 1 (default) the add-constant form
// at float4 rows, where it measured faster (d = 256, paired form, C4 slice:
// 8.361 -> 8.323 us per batch), and the rounding intrinsic at float2 rows,
// where the add-constant form measured slower (d = 128, quad form, C3: 5.607
// -> 5.645 at 2 records per workgroup, 5.314 -> 5.442 at 1); 0 / 2 (A/B
// builds): the intrinsic / the add-constant form everywhere. DESIGN 4.1.
#ifndef HGX_TRAIN_FIXMAGIC
#define HGX_TRAIN_FIXMAGIC 1
#endif

// v rounded to the nearest 2^-44 unit, ties to even (not truncated toward
// zero). v 2^44 is exact in double (24 significant bits, the exponent in
// range), and |v| < kFixLimit bounds it by 2^49, so adding 2^52 + 2^51 lands
// in [2^52, 2^53), where one unit in the last place is 1: the add rounds to
// the nearest integer, ties to even, and the integer is the distance of the
// sum's bit pattern from the constant's (the same exponent field, so a 64-bit
// subtract; negative values borrow from the 2^51 bit). A fused multiply-add
// gives the same bits: the product is exact either way. Denormals and -0
// give 0. Outside the range the value is not the rounded product: the step
// raises its overflow flag there and the sum is never used.
HGX_FIX_HD unsigned long long to_fix_magic(float v) {
  constexpr double kMagic = 6755399441055744.0;  // 2^52 + 2^51
  const double y = (double)v * kFixScale + kMagic;
  return __builtin_bit_cast(unsigned long long, y) -
         __builtin_bit_cast(unsigned long long, kMagic);
}
// the same by the rounding conversion: eight f64 instructions per value on
// gfx950 (cvt, ldexp, rndne, ldexp, floor, fmac, two cvt)
HGX_FIX_HD unsigned long long to_fix_rn(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (unsigned long long)__double2ll_rn((double)v * kFixScale);
#else
  return (unsigned long long)__builtin_llrint((double)v * kFixScale);
#endif
}
// VW: floats per lane of the step's rows (float2 / float4)
template <int VW>
HGX_FIX_HD unsigned long long to_fix(float v) {
  return HGX_TRAIN_FIXMAGIC == 2 || (HGX_TRAIN_FIXMAGIC == 1 && VW == 4) ? to_fix_magic(v)
                                                                         : to_fix_rn(v);
}
