// Runs the shared occlusion / transmission statements of graphaudio_amd/csrc/ga_spatial_direct.hpp, built with a plain host compiler
// (tests/test_spatial_direct_host.py).  Binary float32 on stdin and stdout.
//   occ            : quadruples (occlusion, transmissionLow, transmissionMid, transmissionHigh) -> (s, cM, cL, cH) each
//   walk SR NB     : NB triples (cM, cL, cH), then NB * 128 samples -> NB * 128 samples of x', walked as spatial_direct_kernel walks
//                    one channel: the first block uses its own triple alone, a block is active when its own or the previous triple
//                    is not the identity, the filters start from zero at the first block of a run, other blocks are copied
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ga_spatial_direct.hpp"

using namespace ga;

static std::vector<float> read_all() {
  std::vector<float> v;
  float buf[4096];
  size_t n;
  while ((n = fread(buf, sizeof(float), 4096, stdin)) > 0) v.insert(v.end(), buf, buf + n);
  return v;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::vector<float> in = read_all();
  std::vector<float> out;
  if (!strcmp(argv[1], "occ")) {
    for (size_t i = 0; i + 4 <= in.size(); i += 4) {
      float s;
      SpatialEq c;
      spatial_occlusion(in[i], in[i + 1], in[i + 2], in[i + 3], s, c);
      out.insert(out.end(), {s, c.cM, c.cL, c.cH});
    }
  } else if (!strcmp(argv[1], "walk") && argc >= 4) {
    const SpatialBands K = spatial_bands(atof(argv[2]));
    const size_t nb = (size_t)atoi(argv[3]);
    if (in.size() != nb * 3 + nb * 128) return 3;
    const float* x = in.data() + nb * 3;
    out.assign(x, x + nb * 128);
    float zl = 0.f, zh = 0.f;
    SpatialEq pr{1.0f, 0.0f, 0.0f};
    bool have = false, open = false;
    for (size_t b = 0; b < nb; b++) {
      const SpatialEq cur{in[3 * b], in[3 * b + 1], in[3 * b + 2]};
      if (!have) pr = cur;
      const bool active = !spatial_eq_identity(cur) || !spatial_eq_identity(pr);
      if (active) {
        if (!open) zl = zh = 0.f;
        for (int n = 0; n < 128; n++) out[b * 128 + n] = spatial_direct_step(K, spatial_eq_at(pr, cur, n), x[b * 128 + n], zl, zh);
      }
      open = active;
      have = true;
      pr = cur;
    }
  } else {
    return 2;
  }
  fwrite(out.data(), sizeof(float), out.size(), stdout);
  return 0;
}
