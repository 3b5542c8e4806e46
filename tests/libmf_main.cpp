// Stand-alone host check of graphaudio_amd/csrc/ga_libmf.hpp (option "libm_exact"): ga_cosf / ga_sinf / ga_powf against the cosf /
// sinf / powf of the C library this program is linked with, bit pattern by bit pattern.  Zero mismatches says that this machine's
// libm is of the family the header restates (glibc >= 2.28) and that the restatement is right on the arguments of the sweep.
//
//   libmf_main quick   every 16th float (tests/test_libmf_host.py: a few seconds)
//   libmf_main full    every float, powf for the bases 10, 2.5 and 0.3, and how often libm differs from the double-precision
//                      function rounded once (the table of DESIGN.md section 8; a minute or two on 16 threads)
//   libmf_main gains   the first 32 gains g of a grid of 2^20 floats in [-60, 60] for which powf(10, g / 40) is not the rounded-once
//                      double (tests/test_gpu_libm_exact.py builds its pow scene from them)
//
// Arguments, both signs of each:  the floats of [0, 4.0] (sine, cosine), plus every float within 64 ulp of k pi / 4 (k = 0 .. 5), of
// 2^-12 and of the largest w0 a biquad can form, 2 * 3.14159274f * 24000 / 48000;  the floats y of [0, 1.5] (powf), plus
// y = fl(g / 40f) for the 2^20 gains of the grid.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "ga_libmf.hpp"

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

struct Count {
  std::atomic<uint64_t> n{0}, restated{0}, rounded_once{0};
  std::atomic<uint32_t> first{0};
  std::atomic<bool> has_first{false};
};

static void note(Count& c, uint64_t n, uint64_t bad, uint64_t once, uint32_t first_bad, bool any) {
  c.n += n; c.restated += bad; c.rounded_once += once;
  if (any && !c.has_first.exchange(true)) c.first = first_bad;
}

static constexpr uint32_t kFour = 0x40800000u;      // 4.0f
static constexpr uint32_t kOneHalf = 0x3fc00000u;   // 1.5f
static constexpr int kGainGrid = 1 << 20;

static float grid_gain(int i) { return (float)(-60.0 + 120.0 * (double)i / (double)(kGainGrid - 1)); }

static std::vector<float> neighbourhoods() {
  std::vector<float> c;
  for (int k = 0; k <= 5; k++) c.push_back((float)(k * (3.14159265358979323846 / 4)));
  c.push_back(0x1p-12f);
  c.push_back(2.f * 3.14159274f * 24000.f / 48000.f);
  std::vector<float> v;
  for (float x : c)
    for (int d = -64; d <= 64; d++) {
      const int64_t b = (int64_t)bits(x) + d;
      if (b >= 0) v.push_back(from_bits((uint32_t)b));
    }
  return v;
}

template <class F>
static void parallel(uint64_t n, F&& body) {   // body(lo, hi) over [0, n) in slices
  const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; t++) th.emplace_back([&, t] { body(n * t / nt, n * (t + 1) / nt); });
  for (auto& x : th) x.join();
}

template <class Mine, class Libm, class Once>
static void trig_range(Count& c, uint32_t stride, bool once, Mine mine, Libm libm, Once rounded) {
  parallel((uint64_t)kFour / stride + 1, [&](uint64_t lo, uint64_t hi) {
    uint64_t bad = 0, off = 0;
    uint32_t first = 0;
    for (uint64_t i = lo; i < hi; i++)
      for (uint32_t sign = 0; sign < 2; sign++) {
        const float x = from_bits((uint32_t)(i * stride) | sign << 31);
        const float want = libm(x);
        if (bits(mine(x)) != bits(want) && !bad++) first = bits(x);
        if (once && bits(rounded(x)) != bits(want)) off++;
      }
    note(c, 2 * (hi - lo), bad, off, first, bad != 0);
  });
}

template <class Mine, class Libm>
static void list(Count& c, const std::vector<float>& v, Mine mine, Libm libm) {
  uint64_t bad = 0;
  uint32_t first = 0;
  for (float a : v)
    for (float x : {a, -a})
      if (bits(mine(x)) != bits(libm(x)) && !bad++) first = bits(x);
  note(c, 2 * v.size(), bad, 0, first, bad != 0);
}

static void pow_range(Count& c, float base, uint32_t stride, bool once) {
  parallel((uint64_t)kOneHalf / stride + 1, [&](uint64_t lo, uint64_t hi) {
    uint64_t bad = 0, off = 0;
    uint32_t first = 0;
    for (uint64_t i = lo; i < hi; i++)
      for (uint32_t sign = 0; sign < 2; sign++) {
        const float y = from_bits((uint32_t)(i * stride) | sign << 31);
        const float want = powf(base, y);
        if (bits(ga_powf(base, y)) != bits(want) && !bad++) first = bits(y);
        if (once && bits((float)pow((double)base, (double)y)) != bits(want)) off++;
      }
    note(c, 2 * (hi - lo), bad, off, first, bad != 0);
  });
}

static int report(const char* name, const Count& c, bool once) {
  std::printf("%-14s %12llu arguments, restatement != libm: %llu", name, (unsigned long long)c.n.load(), (unsigned long long)c.restated.load());
  if (c.has_first) std::printf(" (first at bits 0x%08x)", c.first.load());
  if (once) std::printf(", libm != rounded-once double: %llu", (unsigned long long)c.rounded_once.load());
  std::printf("\n");
  return c.restated.load() != 0;
}

static int sweep(bool full) {
  const uint32_t stride = full ? 1 : 16;
  int fails = 0;
  const auto nb = neighbourhoods();
  {
    Count s, co, sn, cn;
    trig_range(s, stride, full, [](float x) { return ga_sinf(x); }, [](float x) { return sinf(x); }, [](float x) { return (float)sin((double)x); });
    trig_range(co, stride, full, [](float x) { return ga_cosf(x); }, [](float x) { return cosf(x); }, [](float x) { return (float)cos((double)x); });
    list(sn, nb, [](float x) { return ga_sinf(x); }, [](float x) { return sinf(x); });
    list(cn, nb, [](float x) { return ga_cosf(x); }, [](float x) { return cosf(x); });
    fails += report("sinf", s, full) + report("cosf", co, full) + report("sinf edges", sn, false) + report("cosf edges", cn, false);
  }
  for (float base : {10.f, 2.5f, 0.3f}) {
    if (base != 10.f && !full) continue;
    Count p;
    pow_range(p, base, stride, full);
    fails += report(("powf(" + std::to_string(base).substr(0, 4) + ")").c_str(), p, full);
  }
  {
    Count g;
    uint64_t bad = 0;
    uint32_t first = 0;
    for (int i = 0; i < kGainGrid; i++) {
      const float y = grid_gain(i) / 40.f;
      if (bits(ga_powf(10.f, y)) != bits(powf(10.f, y)) && !bad++) first = bits(y);
    }
    note(g, kGainGrid, bad, 0, first, bad != 0);
    fails += report("powf gains", g, false);
  }
  // outside the restated domain: the double-precision function rounded once (ga_libmf.hpp says so)
  const bool fb = bits(ga_sinf(1000.f)) == bits((float)sin(1000.0)) && bits(ga_cosf(-120.f)) == bits((float)cos(-120.0)) &&
                  bits(ga_powf(10.f, 50.f)) == bits((float)pow(10.0, 50.0)) && ga_powf(10.f, 0.f) == 1.f && ga_powf(0.f, 2.f) == 0.f &&
                  bits(ga_powf(-2.f, 3.f)) == bits(-8.f) && bits(ga_powf(1e-40f, 0.5f)) == bits((float)pow((double)1e-40f, 0.5));
  if (!fb) { std::printf("FAIL fall-backs\n"); fails++; }
  return fails;
}

static int gains() {
  int found = 0;
  for (int i = 0; i < kGainGrid && found < 32; i++) {
    const float g = grid_gain(i), y = g / 40.f;
    const float lib = powf(10.f, y), once = (float)pow(10.0, (double)y);
    if (bits(lib) != bits(once)) {
      std::printf("gain %.9g bits 0x%08x powf 0x%08x rounded-once 0x%08x restated 0x%08x\n", g, bits(g), bits(lib), bits(once), bits(ga_powf(10.f, y)));
      found++;
    }
  }
  return found > 0 ? 0 : 1;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "quick";
  int fails;
  if (mode == "gains") fails = gains();
  else if (mode == "quick" || mode == "full") fails = sweep(mode == "full");
  else { std::printf("usage: libmf_main quick|full|gains\n"); return 2; }
  std::printf(fails ? "FAILED\n" : "ok\n");
  return fails ? 1 : 0;
}
