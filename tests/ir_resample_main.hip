// Stand-alone device check of graphaudio_amd/csrc/ga_ir_resample.hpp (option "ir_resample"): ir_resample_kernel, run through the
// launcher the library uses (launch_ir_resample of ga_conv.hip), against the host evaluating the same header on the same rows and
// the same table.  The condition is identical bit patterns (tests/test_gpu_ir_resample_kernel.py).
//
// Per rate pair (44.1 -> 48, 48 -> 44.1, 96 -> 48, 8 -> 48, 192 -> 8 kHz): N = 1, 2, 2W-1, 2W, 2W+1; N chosen so that M is tile - 1,
// tile, tile + 1 and 3 tiles + 5 (where upsampling makes M skip the target: the nearest M below for tile - 1, above for the others);
// 1 and 3 channels, and 4096 channels of 16 frames.  Rows are N + 1 floats apart, so they are not aligned.  The inputs are seeded
// values of [-1, 1] with -0.0f, denormals and +-1 among them.  Output rows are M + 3 floats apart; the 3 floats behind a row must
// keep the fill pattern.  One line per case: "<name> <outputs> outputs, device != host: <count>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "ga_kernels.hpp"

using namespace ga;
using namespace ga_irr;

namespace ga {
[[noreturn]] void launch_fail(const char* what) {   // (ga_engine.cpp's is not linked here)
  std::printf("launch_fail: %s\n", what);
  std::exit(2);
}
}  // namespace ga

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); std::exit(1); } } while (0)

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

struct Rng {   // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
};

static float sample(Rng& g) {
  const uint64_t v = g.next();
  switch (v & 15) {
    case 0: return -0.0f;
    case 1: return from_bits((uint32_t)(v >> 40) & 0x007fffffu);                  // a positive denormal (or +0)
    case 2: return from_bits(0x80000000u | ((uint32_t)(v >> 40) & 0x007fffffu));  // a negative one
    case 3: return (v & 16) ? 1.0f : -1.0f;
    default: return (float)((double)(int64_t)(v >> 40) / 8388608.0 - 1.0);        // 24 bits -> [-1, 1), exact
  }
}

template <class T>
struct Dev {
  T* p = nullptr;
  size_t n;
  explicit Dev(size_t n_) : n(n_ ? n_ : 1) { CK(hipMalloc(&p, n * sizeof(T))); CK(hipMemset(p, 0xCD, n * sizeof(T))); }
  ~Dev() { (void)hipFree(p); }
  Dev(const Dev&) = delete;
  Dev& operator=(const Dev&) = delete;
};

static int run_case(const std::string& name, const Plan& p, const double* tab_dev, const std::vector<double>& tab, int channels, int64_t N) {
  const int64_t M = ir_resample_length(N, p.L, p.D);
  const int64_t xs = N + 1, ys = M + 3;
  Rng g{(uint64_t)p.fi * 1000003u + (uint64_t)p.fo * 10007u + (uint64_t)N * 31u + (uint64_t)channels};
  std::vector<float> x((size_t)channels * xs), want((size_t)channels * M), got((size_t)channels * ys);
  for (float& v : x) v = sample(g);
  for (int c = 0; c < channels; c++) ir_resample_row(x.data() + (size_t)c * xs, N, p, tab.data(), want.data() + (size_t)c * M);
  // one float in front of the rows, so that row 0 is not aligned either
  Dev<float> dx(x.size() + 1), dy(got.size() + 1);
  CK(hipMemcpy(dx.p + 1, x.data(), x.size() * sizeof(float), hipMemcpyHostToDevice));
  launch_ir_resample(0, dx.p + 1, xs, N, dy.p + 1, ys, M, channels, p.L, p.D, p.W, p.gain, tab_dev, p.entries());
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  CK(hipMemcpy(got.data(), dy.p + 1, got.size() * sizeof(float), hipMemcpyDeviceToHost));
  size_t bad = 0;
  for (int c = 0; c < channels; c++) {
    for (int64_t m = 0; m < ys; m++) {
      const uint32_t a = bits(got[(size_t)c * ys + m]), b = m < M ? bits(want[(size_t)c * M + m]) : 0xCDCDCDCDu;
      if (a != b && !bad++) std::printf("%s: first difference at channel %d output %lld: device 0x%08x host 0x%08x\n", name.c_str(), c, (long long)m, a, b);
    }
  }
  std::printf("%s %zu outputs, device != host: %zu\n", name.c_str(), (size_t)channels * (size_t)M, bad);
  return bad != 0;
}

// the N whose M is nearest the target: from below (the largest M <= target) or from above (the smallest M >= target)
static int64_t length_for(const Plan& p, int64_t target, bool below) {
  int64_t n = target * p.D / p.L;
  if (n < 1) n = 1;
  if (below) {
    while (n > 1 && ir_resample_length(n, p.L, p.D) > target) n--;
    while (ir_resample_length(n + 1, p.L, p.D) <= target) n++;
  } else {
    while (ir_resample_length(n, p.L, p.D) < target) n++;
    while (n > 1 && ir_resample_length(n - 1, p.L, p.D) >= target) n--;
  }
  return n;
}

int main() {
  static const int pairs[5][2] = {{44100, 48000}, {48000, 44100}, {96000, 48000}, {8000, 48000}, {192000, 8000}};
  int fails = 0;
  for (const auto& pr : pairs) {
    Plan p;
    if (!ir_resample_plan(pr[0], pr[1], p)) { std::printf("no plan for %d -> %d\n", pr[0], pr[1]); return 1; }
    const int tile = ir_resample_tile(p.L, p.D, p.W);
    std::printf("pair %d-%d L %lld D %lld W %d tile %d\n", pr[0], pr[1], (long long)p.L, (long long)p.D, p.W, tile);
    if (tile < 1) return 1;
    const std::vector<double> tab = ir_resample_table(p);
    Dev<double> dtab(tab.size());
    CK(hipMemcpy(dtab.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    const std::string pn = std::to_string(pr[0]) + "-" + std::to_string(pr[1]);
    const int W = p.W;
    const struct { const char* name; int64_t N; } shapes[] = {
        {"N=1", 1}, {"N=2", 2}, {"N=2W-1", 2 * W - 1}, {"N=2W", 2 * W}, {"N=2W+1", 2 * W + 1},
        {"M=tile-1", length_for(p, tile - 1 > 0 ? tile - 1 : 1, true)}, {"M=tile", length_for(p, tile, false)},
        {"M=tile+1", length_for(p, tile + 1, false)}, {"M=3tiles+5", length_for(p, 3 * (int64_t)tile + 5, false)}};
    for (const auto& sh : shapes) fails += run_case(pn + "/" + sh.name + "/ch=3", p, dtab.p, tab, 3, sh.N);
    fails += run_case(pn + "/N=2W+1/ch=1", p, dtab.p, tab, 1, 2 * W + 1);
    fails += run_case(pn + "/N=16/ch=4096", p, dtab.p, tab, 4096, 16);
  }
  std::printf(fails ? "FAILED\n" : "ok\n");
  return fails ? 1 : 0;
}
