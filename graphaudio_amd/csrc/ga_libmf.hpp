// ga_libmf.hpp -- cosf, sinf and powf as glibc >= 2.28 computes them, restated operation for operation (option "libm_exact",
// DESIGN.md section 8 "libm class").  Host and device: the header compiles with plain g++ / clang++ as well as with hipcc.
//
// The reference's MathF.Cos / Sin / Pow are the C library's cosf / sinf / powf.  glibc implements them as short double-precision
// kernels (the "optimized routines" family) whose float result is NOT always the correctly rounded one: 0.03 % .. 0.09 % of the
// arguments of sinf / cosf and 0.006 % of powf's land on the neighbouring float.  Every operation of those kernels is an IEEE double
// multiply, add, conversion or an integer operation, so the same sequence gives the same bits anywhere -- provided no multiply-add
// pair is contracted into an fma: every function below switches contraction off for its own body (clang: a pragma in the body, which
// holds under the HIP default -ffp-contract=fast-honor-pragmas and under on / off; an explicit -ffp-contract=fast disregards pragmas
// by definition and is the one setting this header must not be built with.  gcc: an optimize pragma around the header).
//
// Where the restatement holds, bit for bit (tests/libmf_main.cpp against the machine's libm, tests/libmf_main.hip device against host):
//   ga_cosf / ga_sinf:  |x| < 120.
//   ga_powf:            x finite, normal and > 0; y finite and not 0; |y * log2(x)| < 126 (no overflow, no underflow, no sign).
// Outside it the functions FALL BACK to the double-precision function rounded once -- (float)cos((double)x), (float)sin((double)x),
// (float)pow((double)x, (double)y) -- which is not glibc's result in every last bit (|x| >= 120 goes through a wider reduction in
// glibc, infinities and NaN through its error paths).  The two callers never leave the domain: a biquad's w0 = 2 pi f / fs has f
// clamped to [1, fs / 2], a panner's angle is x pi / 2 with x in [0, 1], and the gain of powf(10, gain / 40) is clamped to [-60, 60].
//
// The tables (16 x {invc, logc} of log2, 32 words of exp2: 512 bytes) are namespace-scope constexpr arrays: constant memory on the
// device, no LDS.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GA_LIBMF_FN __host__ __device__ inline
#else
#define GA_LIBMF_FN inline
#endif

// no contraction inside a function body, for the compilers this header meets
#if defined(__clang__)
#define GA_LIBMF_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define GA_LIBMF_NO_CONTRACT
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

namespace ga_libmf {

// ---- sinf / cosf (glibc sysdeps/ieee754/flt-32/s_sincosf.h, s_sinf.c, s_cosf.c) ----------------------------------------------
constexpr double kHpiInv = 0x1.45F306DC9C883p+23;   // 2 / pi * 2^24
constexpr double kHpi = 0x1.921FB54442D18p0;        // pi / 2
constexpr double kC0 = 0x1p0, kC1 = -0x1.ffffffd0c621cp-2, kC2 = 0x1.55553e1068f19p-5, kC3 = -0x1.6c087e89a359dp-10, kC4 = 0x1.99343027bf8c3p-16;
constexpr double kS1 = -0x1.555545995a603p-3, kS2 = 0x1.1107605230bc4p-7, kS3 = -0x1.994eb3774cf24p-13;

GA_LIBMF_FN uint32_t asuint(float f) {
  uint32_t u;
  memcpy(&u, &f, sizeof u);
  return u;
}
GA_LIBMF_FN float asfloat(uint32_t u) {
  float f;
  memcpy(&f, &u, sizeof f);
  return f;
}
GA_LIBMF_FN uint64_t asuint64(double d) {
  uint64_t u;
  memcpy(&u, &d, sizeof u);
  return u;
}
GA_LIBMF_FN double asdouble(uint64_t u) {
  double d;
  memcpy(&d, &u, sizeof d);
  return d;
}
GA_LIBMF_FN uint32_t abstop12(float x) { return (asuint(x) >> 20) & 0x7ff; }

// `neg`: the second row of glibc's table, the cosine coefficients negated (the sine's are the same in both rows)
GA_LIBMF_FN float sincos_poly(double x, double x2, bool neg, int n) {
  GA_LIBMF_NO_CONTRACT
  if ((n & 1) == 0) {
    const double x3 = x * x2;
    const double s1 = kS2 + x2 * kS3;
    const double x7 = x3 * x2;
    const double s = x + x3 * kS1;
    return (float)(s + x7 * s1);
  }
  const double c0 = neg ? -kC0 : kC0, c1c = neg ? -kC1 : kC1, c2c = neg ? -kC2 : kC2, c3 = neg ? -kC3 : kC3, c4 = neg ? -kC4 : kC4;
  const double x4 = x2 * x2;
  const double c2 = c3 + x2 * c4;
  const double c1 = c0 + x2 * c1c;
  const double x6 = x4 * x2;
  const double c = c1 + x4 * c2c;
  return (float)(c + x6 * c2);
}
GA_LIBMF_FN double reduce_fast(double x, int& n) {
  GA_LIBMF_NO_CONTRACT
  const double r = x * kHpiInv;
  n = ((int32_t)r + 0x800000) >> 24;
  return x - n * kHpi;
}

// ---- powf (glibc sysdeps/ieee754/flt-32/e_powf.c, e_powf_log2_data.c, e_exp2f_data.c) ----------------------------------------
struct Log2Entry { double invc, logc; };
static constexpr Log2Entry kLog2Tab[16] = {
  {0x1.661ec79f8f3bep+0, -0x1.efec65b963019p-2}, {0x1.571ed4aaf883dp+0, -0x1.b0b6832d4fca4p-2},
  {0x1.49539f0f010bp+0, -0x1.7418b0a1fb77bp-2},  {0x1.3c995b0b80385p+0, -0x1.39de91a6dcf7bp-2},
  {0x1.30d190c8864a5p+0, -0x1.01d9bf3f2b631p-2}, {0x1.25e227b0b8eap+0, -0x1.97c1d1b3b7afp-3},
  {0x1.1bb4a4a1a343fp+0, -0x1.2f9e393af3c9fp-3}, {0x1.12358f08ae5bap+0, -0x1.960cbbf788d5cp-4},
  {0x1.0953f419900a7p+0, -0x1.a6f9db6475fcep-5}, {0x1p+0, 0x0p+0},
  {0x1.e608cfd9a47acp-1, 0x1.338ca9f24f53dp-4},  {0x1.ca4b31f026aap-1, 0x1.476a9543891bap-3},
  {0x1.b2036576afce6p-1, 0x1.e840b4ac4e4d2p-3},  {0x1.9c2d163a1aa2dp-1, 0x1.40645f0c6651cp-2},
  {0x1.886e6037841edp-1, 0x1.88e9c2c1b9ff8p-2},  {0x1.767dcf5534862p-1, 0x1.ce0a44eb17bccp-2},
};
constexpr double kA0 = 0x1.27616c9496e0bp-2, kA1 = -0x1.71969a075c67ap-2, kA2 = 0x1.ec70a6ca7baddp-2, kA3 = -0x1.7154748bef6c8p-1, kA4 = 0x1.71547652ab82bp0;
static constexpr uint64_t kExp2Tab[32] = {
  0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull,
  0x3fef72b83c7d517bull, 0x3fef54873168b9aaull, 0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull,
  0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull, 0x3feedea64c123422ull, 0x3feece086061892dull,
  0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull, 0x3feea47eb03a5585ull,
  0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull, 0x3feea11473eb0187ull, 0x3feea589994cce13ull,
  0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull,
  0x3feee89f995ad3adull, 0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull,
  0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full, 0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull,
};
constexpr double kE0 = 0x1.c6af84b912394p-5, kE1 = 0x1.ebfce50fac4f3p-3, kE2 = 0x1.62e42ff0c52d6p-1;
constexpr double kExp2Shift = 0x1.8p52 / 32;

GA_LIBMF_FN double log2_inline(uint32_t ix) {
  GA_LIBMF_NO_CONTRACT
  const uint32_t tmp = ix - 0x3f330000u;
  const int i = (int)((tmp >> (23 - 4)) % 16);
  const uint32_t top = tmp & 0xff800000u;
  const uint32_t iz = ix - top;
  const int k = (int32_t)top >> 23;   // arithmetic shift
  const double invc = kLog2Tab[i].invc, logc = kLog2Tab[i].logc;
  const double z = (double)asfloat(iz);
  const double r = z * invc - 1;
  const double y0 = logc + (double)k;
  const double r2 = r * r;
  double y = kA0 * r + kA1;
  const double p = kA2 * r + kA3;
  const double r4 = r2 * r2;
  double q = kA4 * r + y0;
  q = p * r2 + q;
  y = y * r4 + q;
  return y;
}
GA_LIBMF_FN float exp2_inline(double xd) {
  GA_LIBMF_NO_CONTRACT
  double kd = xd + kExp2Shift;
  const uint64_t ki = asuint64(kd);
  kd -= kExp2Shift;
  const double r = xd - kd;
  uint64_t t = kExp2Tab[ki % 32];
  t += ki << 47;
  const double s = asdouble(t);
  const double z = kE0 * r + kE1;
  const double r2 = r * r;
  double y = kE2 * r + 1;
  y = z * r2 + y;
  y = y * s;
  return (float)y;
}

}  // namespace ga_libmf

GA_LIBMF_FN float ga_sinf(float y) {
  GA_LIBMF_NO_CONTRACT
  using namespace ga_libmf;
  double x = y;
  if (abstop12(y) < abstop12(0x1.921FB6p-1f)) {   // |y| < pi / 4
    if (abstop12(y) < abstop12(0x1p-12f)) return y;
    return sincos_poly(x, x * x, false, 0);
  }
  if (abstop12(y) < abstop12(120.0f)) {
    int n;
    x = reduce_fast(x, n);
    const double s = ((n + 1) & 2) ? -1.0 : 1.0;   // {1, -1, -1, 1}[n & 3]
    return sincos_poly(x * s, x * x, (n & 2) != 0, n);
  }
  return (float)sin((double)y);   // outside the restated domain (see the head of this file)
}

GA_LIBMF_FN float ga_cosf(float y) {
  GA_LIBMF_NO_CONTRACT
  using namespace ga_libmf;
  double x = y;
  if (abstop12(y) < abstop12(0x1.921FB6p-1f)) {
    if (abstop12(y) < abstop12(0x1p-12f)) return 1.0f;
    return sincos_poly(x, x * x, false, 1);
  }
  if (abstop12(y) < abstop12(120.0f)) {
    int n;
    x = reduce_fast(x, n);
    const double s = ((n + 1) & 2) ? -1.0 : 1.0;
    return sincos_poly(x * s, x * x, (n & 2) != 0, n ^ 1);
  }
  return (float)cos((double)y);   // outside the restated domain
}

GA_LIBMF_FN float ga_powf(float x, float y) {
  GA_LIBMF_NO_CONTRACT
  using namespace ga_libmf;
  const uint32_t ix = asuint(x), iy = asuint(y);
  // x zero, subnormal, negative, infinite or NaN; y zero, infinite or NaN (glibc's zeroinfnan): its special cases, not restated
  const bool special = ix - 0x00800000u >= 0x7f800000u - 0x00800000u || 2 * iy - 1 >= 2u * 0x7f800000u - 1;
  if (!special) {
    const double logx = log2_inline(ix);
    const double ylogx = (double)y * logx;
    if ((asuint64(ylogx) >> 47 & 0xffff) < (asuint64(126.0) >> 47)) return exp2_inline(ylogx);
  }
  return (float)pow((double)x, (double)y);   // outside the restated domain
}

#if !defined(__clang__)
#pragma GCC pop_options
#endif
