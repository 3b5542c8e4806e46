// ga_spatial_direct.hpp -- SpatialPannerNode's occlusion / three-band transmission stage (option "spatial_occlusion"; DESIGN.md
// section 2e, "Occlusion and transmission") as one set of __host__ __device__ statements: the occlusion arithmetic (occlusion,
// transmissionLow / Mid / High -> the plain gain s and the EQ triple) is evaluated by the host per block for nodes whose parameters
// it knows (Context::planSpatialPanner) and by spatial_desc_kernel for signal-driven nodes; the one-sample step of the two band
// filters and the mix is what spatial_direct_kernel walks.  The band coefficients are computed once per context on the host.
// Every product and sum here is unfused except where fmaf is written: both builds use -ffp-contract=off, and the functions
// switch contraction off themselves where the compiler has a way to say so, so that the host's and the device's instantiation
// give the same bits.  Nothing here needs the HIP headers: a plain host compiler builds it too
// (tests/test_spatial_direct_host.py).
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GA_DIRECT_HD __host__ __device__
#else
#define GA_DIRECT_HD
#endif
#if defined(__clang__)
#define GA_DIRECT_NOCONTRACT
#define GA_DIRECT_NOCONTRACT_BODY _Pragma("clang fp contract(off)")
#elif defined(__GNUC__)
#define GA_DIRECT_NOCONTRACT __attribute__((optimize("fp-contract=off")))
#define GA_DIRECT_NOCONTRACT_BODY
#else
#define GA_DIRECT_NOCONTRACT
#define GA_DIRECT_NOCONTRACT_BODY
#endif

namespace ga {

struct SpatialEq {      // the EQ triple c_b = (e_M, e_L - e_M, e_H - e_M): x' = cM x + cL lo + cH hi
  float cM, cL, cH;
};
struct SpatialBands {   // one-pole low-pass at f_lo and high-pass at f_hi (bilinear), each coefficient rounded once to float32
  float lb0, lb1, la1;
  float hb0, hb1, ha1;
};

GA_DIRECT_HD inline bool spatial_eq_identity(const SpatialEq& c) { return c.cM == 1.0f && c.cL == 0.0f && c.cH == 0.0f; }

// occlusion (0 = open air, 1 = fully blocked) and the share of each band that passes the obstacle -> s (the largest band factor,
// a plain gain that joins g) and the triple of the remaining EQ.  occ <= 0 (or NaN): s = 1 and the identity (1, 0, 0).
GA_DIRECT_HD GA_DIRECT_NOCONTRACT inline void spatial_occlusion(float occ, float tL, float tM, float tH, float& s, SpatialEq& c) {
  GA_DIRECT_NOCONTRACT_BODY
  float kL = 1.0f, kM = 1.0f, kH = 1.0f;
  if (occ > 0.0f) {
    const float open = 1.0f - occ;
    kL = open + occ * tL;
    kM = open + occ * tM;
    kH = open + occ * tH;
  }
  float m = kL > kM ? kL : kM;
  m = m > kH ? m : kH;
  s = m;
  float eL = 1.0f, eM = 1.0f, eH = 1.0f;
  if (m != 0.0f) {
    eL = kL / m;
    eM = kM / m;
    eH = kH / m;
  }
  c.cM = eM;
  c.cL = eL - eM;
  c.cH = eH - eM;
}

// K = tan(pi f / sampleRate) in double: LP b0 = b1 = K / (1 + K), HP b0 = -b1 = 1 / (1 + K), a1 = (K - 1) / (1 + K) for both
inline SpatialBands spatial_bands(double sampleRate) {
  const double PI = 3.14159265358979323846;
  const double lim = 0.45 * sampleRate;
  const double flo = 800.0 < lim ? 800.0 : lim, fhi = 8000.0 < lim ? 8000.0 : lim;
  const double kl = std::tan(PI * flo / sampleRate), kh = std::tan(PI * fhi / sampleRate);
  SpatialBands b;
  b.lb0 = b.lb1 = (float)(kl / (1.0 + kl));
  b.la1 = (float)((kl - 1.0) / (1.0 + kl));
  b.hb0 = (float)(1.0 / (1.0 + kh));
  b.hb1 = -b.hb0;
  b.ha1 = (float)((kh - 1.0) / (1.0 + kh));
  return b;
}

// the triple of sample n of a block: c_prev + w_n (c_b - c_prev), w_n = (n + 1) / 128 (exact in float32)
GA_DIRECT_HD GA_DIRECT_NOCONTRACT inline SpatialEq spatial_eq_at(const SpatialEq& pr, const SpatialEq& cur, int n) {
  GA_DIRECT_NOCONTRACT_BODY
  const float w = (float)(n + 1) * (1.0f / 128.0f);
  SpatialEq c;
  c.cM = pr.cM + w * (cur.cM - pr.cM);
  c.cL = pr.cL + w * (cur.cL - pr.cL);
  c.cH = pr.cH + w * (cur.cH - pr.cH);
  return c;
}

// one sample: both band filters in transposed direct form II (y = fma(b0, x, z); z = fma(-a1, y, b1 x)), then the mix
GA_DIRECT_HD GA_DIRECT_NOCONTRACT inline float spatial_direct_step(const SpatialBands& k, const SpatialEq& c, float x, float& zl, float& zh) {
  GA_DIRECT_NOCONTRACT_BODY
  const float lo = fmaf(k.lb0, x, zl);
  zl = fmaf(-k.la1, lo, k.lb1 * x);
  const float hi = fmaf(k.hb0, x, zh);
  zh = fmaf(-k.ha1, hi, k.hb1 * x);
  return fmaf(c.cH, hi, fmaf(c.cL, lo, c.cM * x));
}

}  // namespace ga
