// Stand-alone host run of graphaudio_amd/csrc/ga_ir_resample.hpp (option "ir_resample"): tests/test_ir_resample_host.py compares
// what it writes with the float64 model tests/_ir_resample_model.py.
//
//   ir_resample_main plan FI FO                       prints "plan L D W entries", or "refused" (the table would exceed 2^22 entries)
//   ir_resample_main run FI FO CHANNELS N IN OUT      reads CHANNELS rows of N float32 from IN, writes CHANNELS rows of M float32 to OUT
//   ir_resample_main time FI FO CHANNELS N            one host thread on CHANNELS rows of N seeded samples (the figure of DESIGN.md)
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ga_ir_resample.hpp"

using namespace ga_irr;

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (!((mode == "plan" && argc == 4) || (mode == "run" && argc == 8) || (mode == "time" && argc == 6))) {
    std::printf("usage: ir_resample_main plan FI FO | run FI FO CHANNELS N IN OUT | time FI FO CHANNELS N\n");
    return 2;
  }
  Plan p;
  if (!ir_resample_plan(std::atoi(argv[2]), std::atoi(argv[3]), p)) {
    std::printf("refused\nok\n");
    return 0;
  }
  std::printf("plan %lld %lld %d %lld\n", (long long)p.L, (long long)p.D, p.W, (long long)p.entries());
  if (mode == "plan") {
    std::printf("ok\n");
    return 0;
  }
  const int channels = std::atoi(argv[4]);
  const int64_t N = std::atoll(argv[5]);
  if (channels < 1 || N < 0) return 2;
  const int64_t M = ir_resample_length(N, p.L, p.D);
  std::vector<float> x((size_t)channels * (size_t)N), y((size_t)channels * (size_t)M);
  if (mode == "run") {
    FILE* f = std::fopen(argv[6], "rb");
    if (!f || std::fread(x.data(), sizeof(float), x.size(), f) != x.size()) { std::printf("cannot read %s\n", argv[6]); return 1; }
    std::fclose(f);
  } else {
    uint32_t s = 12345u;
    for (float& v : x) { s = s * 1664525u + 1013904223u; v = (float)((double)(int32_t)s / 2147483648.0); }
  }
  const auto t0 = std::chrono::steady_clock::now();
  const std::vector<double> tab = ir_resample_table(p);
  const auto t1 = std::chrono::steady_clock::now();
  for (int c = 0; c < channels; c++) ir_resample_row(x.data() + (size_t)c * (size_t)N, N, p, tab.data(), y.data() + (size_t)c * (size_t)M);
  const auto t2 = std::chrono::steady_clock::now();
  std::printf("M %lld\n", (long long)M);
  if (mode == "time") {
    std::printf("table %.3f ms, rows %.3f ms (one thread)\n", std::chrono::duration<double, std::milli>(t1 - t0).count(),
                std::chrono::duration<double, std::milli>(t2 - t1).count());
  } else {
    FILE* f = std::fopen(argv[7], "wb");
    if (!f || std::fwrite(y.data(), sizeof(float), y.size(), f) != y.size()) { std::printf("cannot write %s\n", argv[7]); return 1; }
    std::fclose(f);
  }
  std::printf("ok\n");
  return 0;
}
