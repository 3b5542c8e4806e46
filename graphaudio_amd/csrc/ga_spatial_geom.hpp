// ga_spatial_geom.hpp -- the geometry of one SpatialPannerNode block (SpatialPannerNode.cs:133-204, ApplyDistanceModel :263-284)
// and the HRIR selection of DESIGN.md section 2e as one set of __host__ __device__ statements: the host evaluates it per block for
// nodes whose parameters it knows (Context::spatialGeometry, ga_plan_nodes.cpp), spatial_desc_kernel evaluates it for nodes whose
// parameters are driven by signals (ga_spatial.hip).  Both builds use -ffp-contract=off.  The two differ only in how acos and pow are
// taken (the `Math` policy): the host keeps the C library's float functions, the device rounds once from double -- the project's
// rule for device transcendentals.  atan2 / asin are double on both sides.
// Nothing here needs the HIP headers: a plain host compiler builds it too (tests/test_spatial_geometry_host.py).
#pragma once
#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GA_SPATIAL_HD __host__ __device__
#else
#define GA_SPATIAL_HD
#endif

namespace ga {

constexpr int kSpatialParams = 17;   // positionX/Y/Z, orientationX/Y/Z, refDistance, maxDistance, rolloffFactor, coneInnerAngle,
                                     // coneOuterAngle, coneOuterGain, spatialBlend, occlusion, transmissionLow/Mid/High
enum : int { kSpatialLinear = 0, kSpatialInverse = 1, kSpatialExponential = 2 };   // SpatialPannerNode.DistanceModelType (:42-47)

struct SpatialGeom {   // what a block's descriptor is made of; idx is NOT clamped to the set (d = j * A + i)
  int idx[4];
  float w[4];
  float g, beta;
};

struct SpatialMathLibm {   // the host path: MathF.Acos / MathF.Pow as the C library's float functions
  static GA_SPATIAL_HD inline float acos_(float x) { return std::acos(x); }
  static GA_SPATIAL_HD inline float pow_(float a, float b) { return std::pow(a, b); }
};
struct SpatialMathDouble {   // the device path: rounded once from double
  static GA_SPATIAL_HD inline float acos_(float x) { return (float)acos((double)x); }
  static GA_SPATIAL_HD inline float pow_(float a, float b) { return (float)pow((double)a, (double)b); }
};

// Math.Clamp / Math.Max in the reference's comparison order (the same statements as clamp_ref / max_ref of ga_kernels.hpp)
GA_SPATIAL_HD inline float spatial_clamp(float v, float mn, float mx) { return v < mn ? mn : (v > mx ? mx : v); }
GA_SPATIAL_HD inline float spatial_max(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

// pv = the 17 parameter values of the block, L = the listener (origin, right, up, ahead: 12 floats), A = hrirAzimuths, D = directions
// of the set.  float32 operation for operation; azimuth / elevation in double from the float32 direction, four bilinear weights
// rounded to float32.
template <class Math>
GA_SPATIAL_HD inline void spatial_geometry(const float* pv, const float* L, int distanceModel, int hrirAzimuths, int D, SpatialGeom& o) {
  float wx = pv[0] - L[0], wy = pv[1] - L[1], wz = pv[2] - L[2];
  float distance = std::sqrt(wx * wx + wy * wy + wz * wz);
  float dx, dy, dz;
  if (distance > 0.0001f) {
    const float invDist = 1.0f / distance;
    wx *= invDist;
    wy *= invDist;
    wz *= invDist;
    dx = wx * L[3] + wy * L[4] + wz * L[5];
    dy = wx * L[6] + wy * L[7] + wz * L[8];
    dz = wx * L[9] + wy * L[10] + wz * L[11];
  } else {
    dx = 0.f;
    dy = 0.f;
    dz = -1.f;
    distance = 0.f;
  }
  float directivity = 1.0f;
  const float innerAngle = pv[9], outerAngle = pv[10], outerGain = pv[11];
  if (innerAngle < 360.f || outerAngle < 360.f) {
    const float oriMag = std::sqrt(pv[3] * pv[3] + pv[4] * pv[4] + pv[5] * pv[5]);
    if (oriMag > 0.0001f) {
      const float invOri = 1.0f / oriMag;
      const float nx = pv[3] * invOri, ny = pv[4] * invOri, nz = pv[5] * invOri;
      float dot = nx * (-wx) + ny * (-wy) + nz * (-wz);
      dot = spatial_clamp(dot, -1.f, 1.f);
      const float angleDeg = Math::acos_(dot) * 180.0f / 3.14159265358979323846f;
      const float absAngle = std::fabs(angleDeg);
      const float halfInner = innerAngle * 0.5f, halfOuter = outerAngle * 0.5f;
      if (absAngle <= halfInner) directivity = 1.0f;
      else if (absAngle >= halfOuter) directivity = outerGain;
      else {
        const float t = (absAngle - halfInner) / (halfOuter - halfInner);
        directivity = 1.0f + t * (outerGain - 1.0f);
      }
    }
  }
  const float refDistance = pv[6], maxDistance = pv[7], rolloff = pv[8];
  // Steam Audio's inverse-distance curve as documented, 1 / max(distance, minDistance) (the library is not available: DESIGN.md section 8)
  const float steam = 1.0f / spatial_max(distance, refDistance);
  const float dc = spatial_clamp(distance, refDistance, maxDistance);
  float attenuation = 1.0f;
  switch (distanceModel) {
    case kSpatialLinear: attenuation = 1.f - rolloff * (dc - refDistance) / (maxDistance - refDistance); break;
    case kSpatialInverse: attenuation = steam; break;
    case kSpatialExponential: attenuation = Math::pow_(dc / refDistance, -rolloff); break;
    default: break;
  }
  attenuation = spatial_clamp(attenuation, 0.f, 1.f);
  o.g = attenuation * (directivity < 0.999f ? directivity : 1.0f);
  o.beta = pv[12];
  // HRIR selection: d = j * A + i, azimuth 360 i / A degrees (0 = -z, +90 = +x), elevation -90 + 180 j / (E - 1)
  const int A = hrirAzimuths > 1 ? hrirAzimuths : 1, E = D / A > 1 ? D / A : 1;
  const double PI = 3.14159265358979323846;
  double az = atan2((double)dx, -(double)dz) * (180.0 / PI);
  if (!(az == az)) az = 0.0;   // (a NaN position: any direction, the gain is NaN as well)
  if (az < 0.0) az += 360.0;
  const double pa = az * (double)A / 360.0;
  double fa0 = floor(pa);
  const double fa = pa - fa0;
  const int i0 = (int)((int64_t)fa0 % A), i1 = (i0 + 1) % A;
  int j0 = 0, j1 = 0;
  double fe = 0.0;
  if (E > 1) {
    const double y = dy < -1.f ? -1.0 : (dy > 1.f ? 1.0 : (double)dy);
    double el = asin(y) * (180.0 / PI);
    if (!(el == el)) el = 0.0;
    const double pe = (el + 90.0) / 180.0 * (double)(E - 1);
    j0 = (int)floor(pe);
    j0 = j0 < 0 ? 0 : (j0 > E - 1 ? E - 1 : j0);
    j1 = j0 + 1 < E - 1 ? j0 + 1 : E - 1;
    fe = j1 == j0 ? 0.0 : pe - (double)j0;
  }
  o.idx[0] = j0 * A + i0;
  o.idx[1] = j0 * A + i1;
  o.idx[2] = j1 * A + i0;
  o.idx[3] = j1 * A + i1;
  o.w[0] = (float)((1.0 - fe) * (1.0 - fa));
  o.w[1] = (float)((1.0 - fe) * fa);
  o.w[2] = (float)(fe * (1.0 - fa));
  o.w[3] = (float)(fe * fa);
}

// the fade decision of a processed block: any of idx, w, g, beta differs from the previous PROCESSED block (a NaN differs from itself)
GA_SPATIAL_HD inline bool spatial_differs(const SpatialGeom& pr, const SpatialGeom& cur) {
  bool fade = !(pr.g == cur.g) || !(pr.beta == cur.beta);
  for (int q = 0; q < 4; q++) fade = fade || pr.idx[q] != cur.idx[q] || !(pr.w[q] == cur.w[q]);
  return fade;
}

}  // namespace ga
