// Stand-alone run of tests/conv_ref.hpp against itself (tests/test_conv_ref_host.py builds it with g++ under the address and
// undefined-behaviour sanitizers, with -ffp-contract=off, and runs it directly; no GPU, no HIP):
//   1. tap_spectrum (the fast transform) against a naive O(N^2) DFT,
//   2. linconv against direct summation written the other way round (per output, indices guarded one by one), with and without history,
//   3. mac_a_bin (layout [block][row], history in rows [0, P-1)) against linconv of every row,
//   4. overlap-save through the float64 transforms -- window, tap_spectrum / N2, inverse, keep the last N2 - P + 1 -- against linconv:
//      the statement of formulation C the device program's bound starts from,
//   5. refmac_f32 against a second scalar loop, written independently (one output at a time), bit for bit: uniform inputs, inputs scaled
//      by 2^-70 (subnormal products), and no history (zeros in front),
//   6. the five plane utilities on small arrays.
// Prints "check <name> ok|FAIL <figures>" per check; exits nonzero if one fails.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "conv_ref.hpp"

using namespace conv_ref;

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
static std::vector<float> uniform(size_t n, uint64_t seed, float scale = 1.f) {
  Rng r{seed};
  std::vector<float> v(n);
  for (float& x : v) x = r.unit() * scale;
  return v;
}

static int failures = 0;
static void check(const char* name, bool ok, double figure, double bound) {
  std::printf("check %s %s %.3e (bound %.3e)\n", name, ok ? "ok" : "FAIL", figure, bound);
  if (!ok) failures++;
}

static void spectrum_against_naive_dft() {
  const int N2 = 1024, P = 65;
  const std::vector<float> hr = uniform(P, 1), hi = uniform(P, 2);
  const std::vector<cd> got = tap_spectrum(hr.data(), hi.data(), P, N2);
  const double pi = 3.14159265358979323846264338327950288;
  double e2 = 0.0, n2 = 0.0;
  for (int j = 0; j < N2; j++) {
    double re = 0.0, im = 0.0;
    for (int p = 0; p < P; p++) {
      const int q = (int)(((int64_t)j * p) % N2);
      const double c = std::cos(2.0 * pi * q / N2), s = -std::sin(2.0 * pi * q / N2);
      re += hr[p] * c - hi[p] * s;
      im += hr[p] * s + hi[p] * c;
    }
    e2 += (got[j].re - re) * (got[j].re - re) + (got[j].im - im) * (got[j].im - im);
    n2 += re * re + im * im;
  }
  const double rel = std::sqrt(e2 / n2);
  check("spectrum_vs_naive_dft", rel <= 1e-12, rel, 1e-12);
}

// y[t] = sum_p X[t - p] H[p], one output at a time, every index guarded where it is used
static void direct(const float* xr, const float* xi, int hist, int nblocks, const float* hr, const float* hi, int P, int nt, double* yr,
                   double* yi) {
  for (int t = 0; t < nt; t++) {
    double re = 0.0, im = 0.0;
    for (int p = 0; p < P; p++) {
      const int blk = t - p;
      if (blk < -hist || blk >= nblocks) continue;
      const double a = xr[hist + blk], b = xi[hist + blk], c = hr[p], d = hi[p];
      re += a * c - b * d;
      im += a * d + b * c;
    }
    yr[t] = re;
    yi[t] = im;
  }
}
static double rel_l2(const double* a, const double* b, const double* c, const double* d, int n) {   // ||(a, c) - (b, d)|| / ||(b, d)||
  double e2 = 0.0, n2 = 0.0;
  for (int i = 0; i < n; i++) {
    e2 += (a[i] - b[i]) * (a[i] - b[i]) + (c[i] - d[i]) * (c[i] - d[i]);
    n2 += b[i] * b[i] + d[i] * d[i];
  }
  return std::sqrt(e2 / n2);
}

static void linconv_against_direct_summation() {
  double worst = 0.0;
  for (int hist : {0, 8, 13}) {
    const int P = 9, nblocks = 21, nt = 24;   // three outputs behind the chunk: the input is zero there
    const std::vector<float> xr = uniform(hist + nblocks, 3 + hist), xi = uniform(hist + nblocks, 4 + hist), hr = uniform(P, 5), hi = uniform(P, 6);
    std::vector<double> ar(nt), ai(nt), br(nt), bi(nt);
    linconv(xr.data(), xi.data(), hist, nblocks, hr.data(), hi.data(), P, nt, ar.data(), ai.data());
    direct(xr.data(), xi.data(), hist, nblocks, hr.data(), hi.data(), P, nt, br.data(), bi.data());
    worst = std::fmax(worst, rel_l2(ar.data(), br.data(), ai.data(), bi.data(), nt));
  }
  check("linconv_vs_direct_summation", worst <= 1e-12, worst, 1e-12);
}

static void mac_a_against_linconv() {
  const int P = 6, n = 10, ty = 12, rp = 8, nrows = 3, tx = ty + P + 4, hist = P - 1;
  std::vector<float> xr = uniform((size_t)tx * rp, 7), xi = uniform((size_t)tx * rp, 8);
  for (int t = hist + n; t < tx; t++)   // behind the chunk: zero rows
    for (int r = 0; r < rp; r++) xr[(size_t)t * rp + r] = xi[(size_t)t * rp + r] = 0.f;
  const std::vector<float> hr = uniform(P, 9), hi = uniform(P, 10);
  std::vector<double> yr((size_t)ty * nrows), yi((size_t)ty * nrows);
  mac_a_bin(xr.data(), xi.data(), rp, hr.data(), hi.data(), P, ty, nrows, yr.data(), yi.data());
  double worst = 0.0;
  for (int r = 0; r < nrows; r++) {
    std::vector<float> sr(hist + n), si(hist + n);
    for (int i = 0; i < hist + n; i++) {
      sr[i] = xr[(size_t)i * rp + r];
      si[i] = xi[(size_t)i * rp + r];
    }
    std::vector<double> br(ty), bi(ty), ar(ty), ai(ty);
    direct(sr.data(), si.data(), hist, n, hr.data(), hi.data(), P, ty, br.data(), bi.data());
    for (int t = 0; t < ty; t++) {
      ar[t] = yr[(size_t)t * nrows + r];
      ai[t] = yi[(size_t)t * nrows + r];
    }
    worst = std::fmax(worst, rel_l2(ar.data(), br.data(), ai.data(), bi.data(), ty));
  }
  check("mac_a_vs_direct_summation", worst <= 1e-12, worst, 1e-12);
}

static void overlap_save_against_linconv() {
  const int N2 = 1024, P = 65, L = N2 - (P - 1), hist = 64, nblocks = L + 37;   // two segments, the second ragged
  const std::vector<float> xr = uniform(hist + nblocks, 11), xi = uniform(hist + nblocks, 12), hr = uniform(P, 13), hi = uniform(P, 14);
  std::vector<double> wr(nblocks), wi(nblocks), gr(nblocks), gi(nblocks);
  linconv(xr.data(), xi.data(), hist, nblocks, hr.data(), hi.data(), P, nblocks, wr.data(), wi.data());
  const std::vector<cd> H = tap_spectrum(hr.data(), hi.data(), P, N2);
  for (int seg = 0; seg * L < nblocks; seg++) {
    const int t0 = seg * L;
    std::vector<cd> w((size_t)N2, cd{0.0, 0.0});
    for (int e = 0; e < N2; e++) {
      const int blk = t0 - (P - 1) + e;
      if (blk >= -hist && blk < nblocks) w[(size_t)e] = cd{xr[hist + blk], xi[hist + blk]};
    }
    fft_radix2(w.data(), N2, -1);
    for (int j = 0; j < N2; j++) {
      const cd a = w[(size_t)j], b{H[(size_t)j].re / N2, H[(size_t)j].im / N2};
      w[(size_t)j] = cd{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
    }
    fft_radix2(w.data(), N2, +1);
    for (int e = P - 1; e < N2 && t0 + e - (P - 1) < nblocks; e++) {
      gr[t0 + e - (P - 1)] = w[(size_t)e].re;
      gi[t0 + e - (P - 1)] = w[(size_t)e].im;
    }
  }
  const double rel = rel_l2(gr.data(), wr.data(), gi.data(), wi.data(), nblocks);
  check("overlap_save_vs_linconv", rel <= 1e-12, rel, 1e-12);
}

// formulation R once more, written on its own: one output at a time, a running pair of accumulators, the window index computed per tap
static void second_refmac(const float* xr, const float* xi, int hist, int nblocks, const float* hr, const float* hi, int P, int nt, float* yr,
                          float* yi) {
  for (int t = 0; t < nt; t++) {
    float accRe = 0.f, accIm = 0.f;
    for (int p = 0; p < P; p++) {
      const int blk = t - p;
      const bool in = blk >= -hist && blk < nblocks;
      const float dr = in ? xr[hist + blk] : 0.f, di = in ? xi[hist + blk] : 0.f;
      const float a = dr * hr[p];
      const float b = di * hi[p];
      const float c = dr * hi[p];
      const float d = di * hr[p];
      const float re = a - b;
      const float im = c + d;
      accRe += re;
      accIm += im;
    }
    yr[t] = accRe;
    yi[t] = accIm;
  }
}
static void refmac_against_second_loop() {
  struct Case { const char* name; int hist; float scale; };
  const Case cases[3] = {{"refmac_vs_second_loop.uniform", 36, 1.f},
                         {"refmac_vs_second_loop.subnormal", 36, 8.470329472543003e-22f /* 2^-70 */},
                         {"refmac_vs_second_loop.nohist", 0, 1.f}};
  for (const Case& c : cases) {
    const int P = 37, nblocks = 50, nt = 52;
    const std::vector<float> xr = uniform(c.hist + nblocks, 15, c.scale), xi = uniform(c.hist + nblocks, 16, c.scale),
                             hr = uniform(P, 17, c.scale), hi = uniform(P, 18, c.scale);
    std::vector<float> ar(nt), ai(nt), br(nt), bi(nt);
    refmac_f32(xr.data(), xi.data(), c.hist, nblocks, hr.data(), hi.data(), P, nt, ar.data(), ai.data());
    second_refmac(xr.data(), xi.data(), c.hist, nblocks, hr.data(), hi.data(), P, nt, br.data(), bi.data());
    int differ = 0, nonzero = 0;
    for (int t = 0; t < nt; t++) {
      differ += std::memcmp(&ar[t], &br[t], 4) != 0;
      differ += std::memcmp(&ai[t], &bi[t], 4) != 0;
      nonzero += ar[t] != 0.f;
    }
    // (the subnormal case means something only if subnormals survive on this host: sums of 2^-140 products are not zero)
    check(c.name, differ == 0 && nonzero > nt / 2, differ, 0.0);
  }
}

static void utilities() {
  int bad = 0;
  {   // hist_copy_b: unequal strides, then zeros
    const int n = 5, ds = 9, ss = 7;
    std::vector<float> src = uniform((size_t)kBins * ss, 19), dst((size_t)kBins * ds, -1.f);
    hist_copy_b(HistJob{dst.data(), src.data(), ds, ss, n});
    for (int k = 0; k < kBins; k++)
      for (int i = 0; i < ds; i++) bad += dst[(size_t)k * ds + i] != (i < n ? src[(size_t)k * ss + i] : -1.f);
    hist_copy_b(HistJob{dst.data(), nullptr, ds, 0, n});
    for (int k = 0; k < kBins; k++)
      for (int i = 0; i < ds; i++) bad += dst[(size_t)k * ds + i] != (i < n ? 0.f : -1.f);
  }
  {   // plane_copy with offsets on both sides
    const int rp = 4, dt = 6, st = 5, n = 2;
    std::vector<float> src = uniform((size_t)kBins * st * rp, 20), dst((size_t)kBins * dt * rp, -1.f);
    plane_copy(dst.data(), dt, 3, src.data(), st, 1, n, rp);
    for (int k = 0; k < kBins; k++)
      for (int t = 0; t < dt; t++)
        for (int r = 0; r < rp; r++) {
          const float want = (t >= 3 && t < 3 + n) ? src[((size_t)k * st + 1 + (t - 3)) * rp + r] : -1.f;
          bad += dst[((size_t)k * dt + t) * rp + r] != want;
        }
  }
  {   // extract_ir
    const int tx = 4, rp = 4, P = 3, nch = 2;
    std::vector<float> x = uniform((size_t)kBins * tx * rp, 21), h((size_t)nch * kBins * P, -1.f);
    extract_ir(h.data(), x.data(), tx, rp, P, nch);
    bad += h[((size_t)1 * kBins + 128) * P + 2] != x[((size_t)128 * tx + 2) * rp + 1];
    bad += h[0] != x[0];
  }
  {   // pair_sum, stale_copy
    std::vector<float> a = uniform(128, 22), b = uniform(128, 23), o(128), d(128);
    pair_sum(o.data(), a.data(), b.data(), 128);
    for (int i = 0; i < 128; i++) bad += o[i] != a[i] + b[i];
    stale_copy(d.data(), a.data(), 0.5f, nullptr);
    for (int i = 0; i < 128; i++) bad += d[i] != a[i] * 0.5f;
    stale_copy(d.data(), a.data(), 0.5f, b.data());
    for (int i = 0; i < 128; i++) bad += d[i] != a[i] * b[i];
    stale_copy(d.data(), nullptr, 0.5f, b.data());
    for (int i = 0; i < 128; i++) bad += d[i] != 0.f;
  }
  check("utilities", bad == 0, bad, 0.0);
}

int main() {
  spectrum_against_naive_dft();
  linconv_against_direct_summation();
  mac_a_against_linconv();
  overlap_save_against_linconv();
  refmac_against_second_loop();
  utilities();
  if (failures) std::printf("%d checks failed\n", failures);
  return failures ? 1 : 0;
}
