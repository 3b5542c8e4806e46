// conv_ref.hpp -- a plain statement of what the fine-partition convolver kernels of graphaudio_amd/csrc/ga_conv.hip compute
// (formulations A, B, R and C, the taps' spectra and the five plane utilities), written from the contracts in ga_kernels.hpp, not from
// the kernels' index arithmetic.  C++17, no HIP, nothing from csrc but the bin count restated below (tests/conv_kernels_main.hip asserts
// it agrees).  Used by tests/conv_ref_main.cpp (the reference against itself, under the sanitizers) and tests/conv_kernels_main.hip
// (the kernels against the reference).
//
//   A          Y[k][t][r] = sum_{p<P} X[k][t + (P-1) - p][r] H[k][p]                 planes [bin][block][row]
//   B / R / C  Y[y0 + j][k][t] = sum_{p<P} X[x][k][t - p] H_j[k][p],  X = 0 in front of block -hist and from block nblocks on;
//              planes [row][bin][block], block t at plane index hist + t
//   taps       hs[c][k][.] = DFT_N2(H[c][k][0..P) zero padded) / N2
// Everything is float64 except refmac_f32, formulation R's own arithmetic: float32, every operation rounded separately, partitions
// ascending from acc = 0 (PartitionedConvolver.cs:154-223).  That loop means what it says only without contraction and fast-math:
// compile with -ffp-contract=off and no flush-to-zero.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#ifdef __FAST_MATH__
#error "conv_ref.hpp: the float32 reference-order loop needs IEEE arithmetic (no -ffast-math)"
#endif

namespace conv_ref {

constexpr int kBins = 129;   // ga::kBins

struct cd {
  double re, im;
};

// ---- formulations B / R / C: one (x-row, bin) sequence against one column's taps ------------------------------------------------------
// x[i], i < hist + nblocks, is block i - hist; blocks outside [-hist, nblocks) are zero.  -> xe[i] = block i - (P - 1), i < nt + P - 1
inline std::vector<float> extend(const float* x, int hist, int nblocks, int P, int nt) {
  std::vector<float> xe((size_t)nt + P - 1, 0.f);
  for (int i = 0; i < nt + P - 1; i++) {
    const int blk = i - (P - 1);
    if (blk >= -hist && blk < nblocks) xe[(size_t)i] = x[hist + blk];
  }
  return xe;
}
// y[t] = sum_{p<P} X[t - p] H[p] for t < nt, float64.  Tap p meets block t - p, which exists for p - hist <= t < nblocks + p: the terms
// outside are products with zero and are left out.
inline void linconv(const float* xr, const float* xi, int hist, int nblocks, const float* hr, const float* hi, int P, int nt, double* yr,
                    double* yi) {
  for (int t = 0; t < nt; t++) yr[t] = yi[t] = 0.0;
  for (int p = 0; p < P; p++) {
    const double a = hr[p], b = hi[p];
    const int lo = p - hist > 0 ? p - hist : 0, hi_t = nblocks + p < nt ? nblocks + p : nt;
    for (int t = lo; t < hi_t; t++) {   // block t - p is x[hist + t - p]
      const double c = xr[hist + t - p], d = xi[hist + t - p];
      yr[t] += c * a - d * b;
      yi[t] += c * b + d * a;
    }
  }
}
// the same sum as formulation R promises it: float32, acc = 0, partitions ascending, re = (xr hr) - (xi hi), im = (xr hi) + (xi hr),
// acc += re / im -- eight separately rounded operations per partition.  (The loops are nested p outside, t inside; every chain acc[t]
// still takes its partitions in ascending order.)
inline void refmac_f32(const float* xr, const float* xi, int hist, int nblocks, const float* hr, const float* hi, int P, int nt, float* yr,
                       float* yi) {
  const std::vector<float> er = extend(xr, hist, nblocks, P, nt), ei = extend(xi, hist, nblocks, P, nt);
  for (int t = 0; t < nt; t++) yr[t] = yi[t] = 0.f;
  for (int p = 0; p < P; p++) {
    const float a = hr[p], b = hi[p];
    const float* cr = er.data() + (P - 1 - p);
    const float* ci = ei.data() + (P - 1 - p);
    for (int t = 0; t < nt; t++) {
      const float m0 = cr[t] * a, m1 = ci[t] * b, m2 = cr[t] * b, m3 = ci[t] * a;
      const float re = m0 - m1, im = m2 + m3;
      yr[t] = yr[t] + re;
      yi[t] = yi[t] + im;
    }
  }
}

// ---- formulation A: one bin.  x planes [tx][rp] of the bin, taps h[P] of the bin, y [ty][nrows] (float64, rows < nrows only) ------------
inline void mac_a_bin(const float* xr, const float* xi, int rp, const float* hr, const float* hi, int P, int ty, int nrows, double* yr,
                      double* yi) {
  for (size_t i = 0; i < (size_t)ty * nrows; i++) yr[i] = yi[i] = 0.0;
  for (int t = 0; t < ty; t++)
    for (int p = 0; p < P; p++) {
      const double a = hr[p], b = hi[p];
      const float* cr = xr + (size_t)(t + (P - 1) - p) * rp;
      const float* ci = xi + (size_t)(t + (P - 1) - p) * rp;
      double* orr = yr + (size_t)t * nrows;
      double* oi = yi + (size_t)t * nrows;
      for (int r = 0; r < nrows; r++) {
        orr[r] += (double)cr[r] * a - (double)ci[r] * b;
        oi[r] += (double)cr[r] * b + (double)ci[r] * a;
      }
    }
}

// ---- transforms ---------------------------------------------------------------------------------------------------------------------
// in-place radix-2 decimation-in-time transform of n = 2^k points, float64; sign = -1: forward, +1: unnormalised inverse
inline void fft_radix2(cd* a, int n, int sign) {
  const double pi = 3.14159265358979323846264338327950288;
  std::vector<cd> w((size_t)n / 2);
  for (int k = 0; k < n / 2; k++) w[(size_t)k] = cd{std::cos(2.0 * pi * k / n), sign * std::sin(2.0 * pi * k / n)};
  for (int i = 1, j = 0; i < n; i++) {
    int bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) {
      const cd t = a[i];
      a[i] = a[j];
      a[j] = t;
    }
  }
  for (int len = 2; len <= n; len <<= 1) {
    const int half = len / 2, step = n / len;
    for (int i = 0; i < n; i += len)
      for (int k = 0; k < half; k++) {
        const cd tw = w[(size_t)k * step], u = a[i + k], v = a[i + k + half];
        const cd t{v.re * tw.re - v.im * tw.im, v.re * tw.im + v.im * tw.re};
        a[i + k] = cd{u.re + t.re, u.im + t.im};
        a[i + k + half] = cd{u.re - t.re, u.im - t.im};
      }
  }
}
// DFT_N2 of the taps h[0..P) zero padded (NOT divided by N2: launch_tap_spectra stores this over N2)
inline std::vector<cd> tap_spectrum(const float* hr, const float* hi, int P, int N2) {
  std::vector<cd> a((size_t)N2, cd{0.0, 0.0});
  for (int p = 0; p < P; p++) a[(size_t)p] = cd{hr[p], hi[p]};
  fft_radix2(a.data(), N2, -1);
  return a;
}

// ---- the plane utilities (float32 in, float32 out: copies, one product, one sum) ---------------------------------------------------
struct HistJob {   // ga::HistJobB on host arrays: kBins runs of n floats; src == nullptr: zeros
  float* dst;
  const float* src;
  int dst_stride, src_stride, n;
};
inline void hist_copy_b(const HistJob& j) {
  for (int k = 0; k < kBins; k++)
    for (int i = 0; i < j.n; i++) j.dst[(size_t)k * j.dst_stride + i] = j.src ? j.src[(size_t)k * j.src_stride + i] : 0.f;
}
// dst[k][dst_t0 + i][:] = src[k][src_t0 + i][:] for i < n (src == nullptr: zeros); planes [kBins][*_t][rp]
inline void plane_copy(float* dst, int dst_t, int dst_t0, const float* src, int src_t, int src_t0, int n, int rp) {
  for (int k = 0; k < kBins; k++)
    for (int i = 0; i < n; i++)
      for (int r = 0; r < rp; r++)
        dst[((size_t)k * dst_t + dst_t0 + i) * rp + r] = src ? src[((size_t)k * src_t + src_t0 + i) * rp + r] : 0.f;
}
// h[c][k][p] = x[k][p][c] for c < nch
inline void extract_ir(float* h, const float* x, int tx, int rp, int P, int nch) {
  for (int c = 0; c < nch; c++)
    for (int k = 0; k < kBins; k++)
      for (int p = 0; p < P; p++) h[((size_t)c * kBins + k) * P + p] = x[((size_t)k * tx + p) * rp + c];
}
inline void pair_sum(float* out, const float* a, const float* b, int64_t n) {
  for (int64_t i = 0; i < n; i++) out[i] = a[i] + b[i];
}
// dst[0..128) = src x scale, or src x curve where there is a curve, or zeros without a source
inline void stale_copy(float* dst, const float* src, float scale, const float* curve) {
  for (int i = 0; i < 128; i++) dst[i] = src ? src[i] * (curve ? curve[i] : scale) : 0.f;
}

}  // namespace conv_ref
