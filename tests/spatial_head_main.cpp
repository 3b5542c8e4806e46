// Stand-alone host check of graphaudio_amd/csrc/ga_spatial_head.hpp (the built-in HRIR set of SpatialPannerNode), built with a plain
// host compiler.  stdin: one request per line -- sample rate, head radius, channel.  stdout per request: T, the gain bound of the
// channel, then the channel's T taps as the hexadecimal bit patterns of the float32 values.
#include <cstdio>
#include <cstring>
#include <vector>

#include "ga_spatial_head.hpp"

int main() {
  double fs, a;
  int channel;
  while (std::scanf("%lf %lf %d", &fs, &a, &channel) == 3) {
    if (channel < 0 || channel >= 2 * ga::kSpatialHeadDirs) return 2;
    const int T = ga::spatial_head_taps(fs, a);
    const ga::SpatialHeadEar e = ga::spatial_head_ear(fs, a, channel);
    std::vector<float> h((size_t)T);   // (its own allocation: a tap index past T would be an out-of-bounds write the sanitizer sees)
    for (int k = 0; k < T; k++) h[(size_t)k] = ga::spatial_head_tap(e, k);
    std::printf("%d %.17g", T, ga::spatial_head_abs_sum_bound(e));
    for (int k = 0; k < T; k++) {
      unsigned u;
      std::memcpy(&u, &h[(size_t)k], 4);
      std::printf(" %08x", u);
    }
    std::printf("\n");
  }
  return 0;
}
