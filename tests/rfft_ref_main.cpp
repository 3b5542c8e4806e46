// tests/rfft_ref.hpp against itself: built with g++ under the address and undefined-behaviour sanitizers and run directly (no GPU, no
// HIP) by tests/test_rfft_ref_host.py.  One line per check, "check <name> ok|FAIL <figures>"; exit status 1 if any check fails.
//   forward_vs_naive, inverse_vs_naive   the radix-2 path against the O(N^2) sums of the contract, 1e-12 relative
//   roundtrip                            inverse(forward(x)) = [x | 0]
//   ola_vs_linear_convolution            overlap-add of inverse(forward(x_t) H) over several blocks, with an incoming overlap, against
//                                        direct linear convolution with a 129-tap filter (the longest a 256-point transform carries), 1e-12
//   layouts                              index_a / index_b enumerate their planes once each, in the order the contract names
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rfft_ref.hpp"

namespace rr = rfft_ref;
using rr::cd;

static int failures = 0;
static void check(const char* name, bool ok, double figure, const char* what) {
  std::printf("check %s %s %s %.3e\n", name, ok ? "ok" : "FAIL", what, figure);
  if (!ok) failures++;
}
struct Rng {   // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  float unit() { return (float)((double)(int64_t)(next() >> 40) / 8388608.0 - 1.0); }
};

int main() {
  Rng rng{20240601};
  // forward, inverse against the naive sums
  {
    double worst = 0.0;
    for (int rep = 0; rep < 8; rep++) {
      float x[rr::kBlock];
      double d[rr::kBlock];
      for (int n = 0; n < rr::kBlock; n++) d[n] = x[n] = rng.unit();
      cd X[rr::kBins], Xn[rr::kBins];
      rr::forward(x, X);
      rr::rdft256_naive(d, rr::kBlock, Xn);
      double e = 0.0, m = 0.0;
      for (int k = 0; k < rr::kBins; k++) {
        e = std::max(e, std::hypot(X[k].re - Xn[k].re, X[k].im - Xn[k].im));
        m = std::max(m, std::hypot(Xn[k].re, Xn[k].im));
      }
      worst = std::max(worst, e / m);
    }
    cd Z[rr::kBins];
    rr::forward(nullptr, Z);
    bool silent = true;
    for (int k = 0; k < rr::kBins; k++) silent = silent && Z[k].re == 0.0 && Z[k].im == 0.0;
    check("forward_vs_naive", worst <= 1e-12 && silent, worst, "max |X - naive| / max |naive|");
  }
  {
    double worst = 0.0;
    for (int rep = 0; rep < 8; rep++) {
      cd Y[rr::kBins];
      for (int k = 0; k < rr::kBins; k++) Y[k] = cd{rng.unit(), rng.unit()};   // Im Y[0], Im Y[128] non-zero: ignored
      double y[rr::kN], yn[rr::kN];
      rr::inverse(Y, y);
      rr::inverse_naive(Y, yn);
      double e = 0.0, m = 0.0;
      for (int n = 0; n < rr::kN; n++) {
        e = std::max(e, std::fabs(y[n] - yn[n]));
        m = std::max(m, std::fabs(yn[n]));
      }
      worst = std::max(worst, e / m);
    }
    check("inverse_vs_naive", worst <= 1e-12, worst, "max |y - naive| / max |naive|");
  }
  {
    double worst = 0.0;
    for (int rep = 0; rep < 8; rep++) {
      float x[rr::kBlock];
      for (int n = 0; n < rr::kBlock; n++) x[n] = rng.unit();
      cd X[rr::kBins];
      double y[rr::kN];
      rr::forward(x, X);
      rr::inverse(X, y);
      for (int n = 0; n < rr::kN; n++) worst = std::max(worst, std::fabs(y[n] - (n < rr::kBlock ? (double)x[n] : 0.0)));
    }
    check("roundtrip", worst <= 1e-12, worst, "max |inverse(forward(x)) - [x | 0]|");
  }
  {
    const int nb = 5, taps = 129;
    std::vector<double> x((size_t)nb * rr::kBlock), h(taps), ov(rr::kBlock);
    std::vector<float> xf(x.size());
    for (size_t i = 0; i < x.size(); i++) x[i] = xf[i] = rng.unit();
    for (double& v : h) v = rng.unit();
    for (double& v : ov) v = rng.unit();
    cd H[rr::kBins];
    rr::rdft256(h.data(), taps, H);
    std::vector<double> y((size_t)nb * rr::kN), out(x.size()), ovo(rr::kBlock);
    for (int t = 0; t < nb; t++) {
      cd X[rr::kBins], Y[rr::kBins];
      rr::forward(xf.data() + (size_t)t * rr::kBlock, X);
      for (int k = 0; k < rr::kBins; k++) Y[k] = cd{X[k].re * H[k].re - X[k].im * H[k].im, X[k].re * H[k].im + X[k].im * H[k].re};
      rr::inverse(Y, y.data() + (size_t)t * rr::kN);
    }
    rr::overlap_add(y.data(), nb, ov.data(), out.data(), ovo.data());
    double worst = 0.0, peak = 0.0;
    for (int i = 0; i < (nb + 1) * rr::kBlock; i++) {   // the nb blocks, then the outgoing overlap
      double want = i < rr::kBlock ? ov[i] : 0.0;
      for (int j = 0; j < taps; j++)
        if (i - j >= 0 && i - j < nb * rr::kBlock) want += h[j] * x[(size_t)(i - j)];
      const double got = i < nb * rr::kBlock ? out[(size_t)i] : ovo[(size_t)(i - nb * rr::kBlock)];
      worst = std::max(worst, std::fabs(got - want));
      peak = std::max(peak, std::fabs(want));
    }
    check("ola_vs_linear_convolution", worst <= 1e-12 * peak, worst / peak, "max error / peak");
  }
  {
    const int hist = 3, n = 5, T = 11, rp = 4, rows = 3;
    bool ok = true;
    // A: bins outermost, then blocks, rows fastest;  B: rows outermost, then bins, blocks fastest
    for (int k = 0; k < rr::kBins; k++)
      for (int t = 0; t < n; t++)
        for (int r = 0; r < rp; r++) {
          const size_t a = rr::index_a(k, t, r, hist, T, rp);
          ok = ok && a < (size_t)rr::kBins * T * rp && a % rp == (size_t)r && a / rp % T == (size_t)(hist + t) && a / rp / T == (size_t)k;
        }
    for (int r = 0; r < rows; r++)
      for (int k = 0; k < rr::kBins; k++)
        for (int t = 0; t < n; t++) {
          const size_t b = rr::index_b(r, k, t, hist, T);
          ok = ok && b < (size_t)rows * rr::kBins * T && b % T == (size_t)(hist + t) && b / T % rr::kBins == (size_t)k && b / T / rr::kBins == (size_t)r;
        }
    check("layouts", ok, 0.0, "index_a, index_b");
  }
  return failures ? 1 : 0;
}
