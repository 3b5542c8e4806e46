// ga_spatial_head.hpp -- the built-in HRIR set of SpatialPannerNode (options "spatial_builtin_hrir", "spatial_head_radius"; DESIGN.md
// section 2e, "The built-in set"): Brown & Duda's structural model of a rigid spherical head -- per ear a delay that depends on the angle
// of incidence and a one-pole one-zero head-shadow filter -- sampled on the 72 x 25 grid of section 2e at the context's rate.  The set
// is this library's own DEFINITION, not a measurement: tests/_spatial_head_model.py restates it in numpy and is what the tests hold
// both instantiations to.  One set of __host__ __device__ statements: spatial_head_kernel (ga_spatial.hip) evaluates a tap per lane,
// the host evaluates the length, the gain bound and (tests/spatial_head_main.cpp) single taps.  Everything is double and a tap is
// rounded to float32 once.  Nothing here needs the HIP headers: a plain host compiler builds it too.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GA_SPATIAL_HEAD_HD __host__ __device__
#else
#define GA_SPATIAL_HEAD_HD
#endif

namespace ga {

constexpr int kSpatialHeadAzimuths = 72;      // A: azimuth 360 i / A degrees
constexpr int kSpatialHeadElevations = 25;    // E: elevation -90 + 180 j / (E - 1) degrees
constexpr int kSpatialHeadDirs = kSpatialHeadAzimuths * kSpatialHeadElevations;   // D: d = j * A + i, channel 2 d = left ear, 2 d + 1 = right ear
constexpr int kSpatialHeadMaxTaps = 512;      // (= kSpatialMaxTaps, ga_kernels.hpp)
constexpr int kSpatialHeadHalfWidth = 8;      // the fractional delay: a Hann-windowed sinc of this half-width
constexpr double kSpatialHeadSound = 343.0;   // c, m/s
constexpr double kSpatialHeadPi = 3.14159265358979323846;
constexpr double kSpatialHeadRadiusDefault = 0.0875, kSpatialHeadRadiusMin = 0.04, kSpatialHeadRadiusMax = 0.20;

struct SpatialHeadEar {   // one channel of the set: h[k] = sum_n p[n] g[k - n]
  double d;               // centre of the fractional-delay kernel p, in samples: 8 + fs tau(theta)
  double b0, c1, r;       // the head shadow's impulse response: g[0] = b0, g[n] = c1 r^(n - 1) with c1 = b1 - a1 b0, r = -a1
};

// a1 of the bilinear transform of (alpha s + beta) / (s + beta), beta = 2 c / a: it does not depend on the direction
GA_SPATIAL_HEAD_HD inline double spatial_head_a1(double fs, double a) {
  const double beta = 2.0 * kSpatialHeadSound / a;
  return (beta - 2.0 * fs) / (beta + 2.0 * fs);
}

// T = min(512, 8 ceil((Dmax + 16 + L) / 8)): Dmax = ceil(fs (a / c) (1 + pi / 2)) the longest delay, 16 the kernel's width, L the
// smallest n with |a1|^n <= 2^-14.  Where the cap bites (192 kHz with a = 0.15, say) the shadow filter's tail is cut off at tap 512.
GA_SPATIAL_HEAD_HD inline int spatial_head_taps(double fs, double a) {
  const double dmax = std::ceil(fs * (a / kSpatialHeadSound) * (1.0 + 0.5 * kSpatialHeadPi));
  const double r = std::fabs(spatial_head_a1(fs, a));
  int L = 0;
  for (double q = 1.0; q > 1.0 / 16384.0 && L < 8 * kSpatialHeadMaxTaps; q *= r) L++;
  const double t = 8.0 * std::ceil((dmax + 2.0 * kSpatialHeadHalfWidth + (double)L) / 8.0);
  return t < (double)kSpatialHeadMaxTaps ? (int)t : kSpatialHeadMaxTaps;
}

// channel -> the ear's delay and shadow filter.  u = (sin az cos el, sin el, -cos az cos el) is the direction in listener space; the
// ears sit on the x axis (right ear +x, left ear -x), theta = acos(clamp(u . e, -1, 1)) is the angle of incidence.
GA_SPATIAL_HEAD_HD inline SpatialHeadEar spatial_head_ear(double fs, double a, int channel) {
  const int dir = channel >> 1, i = dir % kSpatialHeadAzimuths, j = dir / kSpatialHeadAzimuths;
  const double az = (360.0 * i / kSpatialHeadAzimuths) * (kSpatialHeadPi / 180.0);
  const double el = (-90.0 + 180.0 * j / (kSpatialHeadElevations - 1)) * (kSpatialHeadPi / 180.0);
  const double ux = std::sin(az) * std::cos(el);
  double dot = (channel & 1) ? ux : -ux;
  dot = dot < -1.0 ? -1.0 : (dot > 1.0 ? 1.0 : dot);
  const double theta = std::acos(dot);
  const double ac = a / kSpatialHeadSound;
  const double tau = theta < 0.5 * kSpatialHeadPi ? ac * (1.0 - std::cos(theta)) : ac * (1.0 + theta - 0.5 * kSpatialHeadPi);
  const double alpha = 1.05 + 0.95 * std::cos(theta * (180.0 / 150.0));
  const double beta = 2.0 * kSpatialHeadSound / a;
  const double b0 = (beta + 2.0 * fs * alpha) / (beta + 2.0 * fs);
  const double b1 = (beta - 2.0 * fs * alpha) / (beta + 2.0 * fs);
  const double a1 = spatial_head_a1(fs, a);
  SpatialHeadEar e;
  e.d = (double)kSpatialHeadHalfWidth + fs * tau;
  e.b0 = b0;
  e.c1 = b1 - a1 * b0;
  e.r = -a1;
  return e;
}

// r^m for an integer m >= 0 by squaring: the same products on the host and on the device
GA_SPATIAL_HEAD_HD inline double spatial_head_ipow(double r, int m) {
  double acc = 1.0;
  for (; m > 0; m >>= 1, r *= r)
    if (m & 1) acc *= r;
  return acc;
}

// p[n] = sinc(n - d) 0.5 (1 + cos(pi (n - d) / 8)) for |n - d| < 8, else 0
GA_SPATIAL_HEAD_HD inline double spatial_head_kernel_at(double d, int n) {
  const double x = (double)n - d;
  if (!(std::fabs(x) < (double)kSpatialHeadHalfWidth)) return 0.0;
  const double px = kSpatialHeadPi * x;
  const double sinc = x == 0.0 ? 1.0 : std::sin(px) / px;
  return sinc * 0.5 * (1.0 + std::cos(px / (double)kSpatialHeadHalfWidth));
}

// tap k of the ear: sum over ascending n of p[n] g[k - n], in double, rounded once
GA_SPATIAL_HEAD_HD inline float spatial_head_tap(const SpatialHeadEar& e, int k) {
  int n0 = (int)std::floor(e.d) - kSpatialHeadHalfWidth;   // (|n - d| < 8 holds for at most 16 n from here on: d >= 8, so n0 >= 0)
  if (n0 < 0) n0 = 0;
  double acc = 0.0;
  for (int n = n0; n <= n0 + 2 * kSpatialHeadHalfWidth && n <= k; n++) {
    const double p = spatial_head_kernel_at(e.d, n);
    if (p == 0.0) continue;
    const int m = k - n;
    const double g = m == 0 ? e.b0 : e.c1 * spatial_head_ipow(e.r, m - 1);
    acc += p * g;
  }
  return (float)acc;
}

// what sum_k |h[k]| of the ear cannot exceed: sum |p| sum |g| (the loop-gain estimate's bound for a node on the set)
GA_SPATIAL_HEAD_HD inline double spatial_head_abs_sum_bound(const SpatialHeadEar& e) {
  const int n0 = (int)std::floor(e.d) - kSpatialHeadHalfWidth;
  double sp = 0.0;
  for (int n = n0; n <= n0 + 2 * kSpatialHeadHalfWidth; n++) sp += std::fabs(spatial_head_kernel_at(e.d, n));
  const double r = std::fabs(e.r);
  const double sg = std::fabs(e.b0) + (r < 1.0 ? std::fabs(e.c1) / (1.0 - r) : 1e30);
  return sp * sg;
}

}  // namespace ga
