// Stand-alone run of tests/coarse_ref.hpp against itself (tests/test_coarse_ref_host.py builds it with g++ under the address and
// undefined-behaviour sanitizers and runs it directly; no GPU, no HIP):
//   1. the fast transform inside ref_spectrum against a naive O(N^2) DFT of one full window,
//   2. ref_inv(ref_mac(ref_fwd(x), ref_fwd(h))) against direct float64 convolution: a 3-partition response, a 5-block signal with history.
// Prints "check <name> ok|FAIL <figures>" per check; exits nonzero if one fails.
#include <cstdio>
#include <cstdlib>

#include "coarse_ref.hpp"

using namespace coarse_ref;

struct Rng {   // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  float unit() { return (float)((double)(int64_t)(next() >> 40) / 8388608.0 - 1.0); }   // 24 bits -> [-1, 1), exact
};

static int failures = 0;
static void check(const char* name, bool ok, double figure, double bound) {
  std::printf("check %s %s %.3e (bound %.3e)\n", name, ok ? "ok" : "FAIL", figure, bound);
  if (!ok) failures++;
}

static void spectrum_against_naive_dft() {
  Rng rng{1};
  std::vector<double> w(N);
  for (double& v : w) v = rng.unit();
  const std::vector<cd> got = ref_spectrum(w.data());
  const double pi = 3.14159265358979323846264338327950288;
  std::vector<double> co(N), si(N);
  for (int k = 0; k < N; k++) {
    co[k] = std::cos(2.0 * pi * k / N);
    si[k] = std::sin(2.0 * pi * k / N);
  }
  std::vector<cd> X(NB + 1);
  const double* wp = w.data();
  const double* cp = co.data();
  const double* sp = si.data();
  for (int k = 0; k <= NB; k++) {
    double re = 0.0, im = 0.0;
    for (int n = 0; n < N; n++) {
      const int q = (int)(((int64_t)k * n) & (N - 1));
      re += wp[n] * cp[q];
      im -= wp[n] * sp[q];
    }
    X[k] = cd{re, im};
  }
  std::vector<cd> want(NB);
  pack_bins(X.data(), want.data());
  double e2 = 0.0, n2 = 0.0;
  for (int b = 0; b < NB; b++) {
    e2 += (got[b].re - want[b].re) * (got[b].re - want[b].re) + (got[b].im - want[b].im) * (got[b].im - want[b].im);
    n2 += want[b].re * want[b].re + want[b].im * want[b].im;
  }
  // both sides are float64: the naive sum of 16,384 terms carries ~ sqrt(N) 2^-53, the fast one ~ log2(N) 2^-53
  const double rel = std::sqrt(e2 / n2);
  check("spectrum_vs_naive_dft", rel <= 1e-12, rel, 1e-12);
}

static void chain_against_direct_convolution() {
  Rng rng{2};
  const int P = 3, nT = 5;
  const int64_t taps = 2 * (int64_t)CB + 1000, n = 4 * (int64_t)CB + 384, hl = (int64_t)P * CB;
  std::vector<float> h((size_t)taps), hist((size_t)hl), in((size_t)n);
  for (float& v : h) v = rng.unit();
  for (float& v : hist) v = rng.unit();
  for (float& v : in) v = rng.unit();
  XRow hr;
  hr.in = h.data();
  hr.nvalid = taps;
  hr.n_frames = P;
  hr.u0 = 1;            // window p + 1 starts at partition p; its second half is zero
  hr.flags = 1;
  hr.scale = 1.0f / 65536.0f;
  XRow xr;
  xr.hist = hist.data();
  xr.hist_len = hl;
  xr.in = in.data();
  xr.nvalid = n;
  xr.u0 = -(P - 1);
  xr.n_frames = nT + P - 1;
  const std::vector<cd> H = ref_fwd(hr), X = ref_fwd(xr);
  MacJob<double> J;
  J.P = P;
  J.t0 = 0;
  J.n_t = nT;
  J.u_lo = -(P - 1);
  J.u_hi = nT - 1;
  MacTerm<double> term{X.data(), P - 1, {}};
  term.h[0] = H.data();
  J.terms.push_back(term);
  std::vector<cd> Y((size_t)nT * NB);
  for (int t = 0; t < nT; t++) ref_mac(J, 0, t, Y.data() + (size_t)t * NB);
  OutDesc o;
  o.nvalid = n;
  o.rows = {0};
  o.n_y = nT;
  const std::vector<double> got = ref_inv(o, Y.data(), nT);
  // direct: y[i] = sum_k h[k] s[i - k] over history ++ chunk
  std::vector<double> s((size_t)(hl + n)), hd((size_t)taps);
  for (int64_t i = 0; i < hl; i++) s[(size_t)i] = hist[(size_t)i];
  for (int64_t i = 0; i < n; i++) s[(size_t)(hl + i)] = in[(size_t)i];
  for (int64_t k = 0; k < taps; k++) hd[(size_t)k] = h[(size_t)k];
  double worst = 0.0, peak = 0.0;
  const double* sp = s.data();
  const double* hp = hd.data();
  for (int64_t i = 0; i < n; i++) {
    double acc = 0.0;
    const double* si = sp + hl + i;
    for (int64_t k = 0; k < taps; k++) acc += hp[k] * si[-k];
    peak = std::fmax(peak, std::fabs(acc));
    worst = std::fmax(worst, std::fabs(acc - got[(size_t)i]));
  }
  check("chain_vs_direct_convolution", got.size() == (size_t)n && worst <= 1e-12 * peak, worst / peak, 1e-12);
}

int main() {
  spectrum_against_naive_dft();
  chain_against_direct_convolution();
  if (failures) std::printf("%d checks failed\n", failures);
  return failures ? 1 : 0;
}
