// A stand-alone host program around graphaudio_amd/csrc/ga_spatial_geom.hpp (tests/test_spatial_geometry_host.py builds it with a
// plain host compiler).  stdin: one parameter set per line -- distance model, hrirAzimuths, directions, 12 listener floats, 17
// parameter values.  stdout: per line, for the host's instantiation (C library float acos / pow) and then for the device's
// (rounded once from double): four indices, and the bit patterns of the four weights, g and beta.
#include <cstdio>
#include <cstring>

#include "ga_spatial_geom.hpp"

static unsigned bits(float f) {
  unsigned u;
  std::memcpy(&u, &f, sizeof u);
  return u;
}

static void show(const ga::SpatialGeom& o) {
  for (int q = 0; q < 4; q++) std::printf("%d ", o.idx[q]);
  for (int q = 0; q < 4; q++) std::printf("%08x ", bits(o.w[q]));
  std::printf("%08x %08x ", bits(o.g), bits(o.beta));
}

int main() {
  int model, A, D;
  while (std::scanf("%d %d %d", &model, &A, &D) == 3) {
    float L[12], pv[ga::kSpatialParams];
    for (float& v : L)
      if (std::scanf("%f", &v) != 1) return 2;
    for (float& v : pv)
      if (std::scanf("%f", &v) != 1) return 2;
    ga::SpatialGeom a, b;
    ga::spatial_geometry<ga::SpatialMathLibm>(pv, L, model, A, D, a);
    ga::spatial_geometry<ga::SpatialMathDouble>(pv, L, model, A, D, b);
    show(a);
    show(b);
    std::printf("\n");
  }
  return 0;
}
