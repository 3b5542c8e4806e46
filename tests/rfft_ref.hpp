// rfft_ref.hpp -- a plain float64 statement of what the 256-point real-FFT kernels of graphaudio_amd/csrc/ga_rfft.hip compute, written
// from the contracts in ga_kernels.hpp, not from the kernels' lane arithmetic.  C++17, no HIP, nothing from csrc but the two constants
// restated below (tests/rfft_ref_kernels_main.hip asserts they agree).  Used by tests/rfft_ref_main.cpp (the reference against itself,
// under the sanitizers) and tests/rfft_ref_kernels_main.hip (the kernels against the reference).
//
//   forward   block t of a row (128 samples, zero padded to 256):  X[k] = sum_{n<128} x[128 t + n] e^{-2 pi i k n / 256},  k = 0..128,
//             unscaled, Im X[0] = Im X[128] = 0.  A null row is silence.
//   inverse   y[n] = (1/256) (Re Y[0] + (-1)^n Re Y[128] + 2 sum_{k=1..127} Re(Y[k] e^{+2 pi i k n / 256})),  n < 256; Im Y[0] and
//             Im Y[128] are ignored.  head = y[0..128), tail = y[128..256);  out_t = head_t + tail_{t-1}, tail_{-1} = the incoming
//             overlap; the outgoing overlap is the last block's tail.
//   layouts   A: planes [bin][block][row], block t at hist + t, rp rows;  B: planes [row][bin][block], block t at hist + t.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

#include "conv_ref.hpp"

namespace rfft_ref {

using conv_ref::cd;
constexpr int kBlock = 128;   // ga::kBlock
constexpr int kBins = 129;    // ga::kBins
constexpr int kN = 2 * kBlock;

// X[k], k = 0..128, of the real sequence x[0..len) zero padded to 256 points (len <= 256)
inline void rdft256(const double* x, int len, cd* X) {
  cd a[kN];
  for (int n = 0; n < kN; n++) a[n] = cd{n < len ? x[n] : 0.0, 0.0};
  conv_ref::fft_radix2(a, kN, -1);
  for (int k = 0; k < kBins; k++) X[k] = a[k];
  X[0].im = 0.0;   // (sums of real numbers: the transform leaves exact zeros there anyway)
  X[kBlock].im = 0.0;
}
// forward of one block: x = 128 floats, or nullptr for silence
inline void forward(const float* x, cd* X) {
  double d[kBlock];
  for (int n = 0; n < kBlock; n++) d[n] = x ? (double)x[n] : 0.0;
  rdft256(d, x ? kBlock : 0, X);
}
// inverse of one spectrum Y[0..128] -> y[0..256)
inline void inverse(const cd* Y, double* y) {
  cd a[kN];
  a[0] = cd{Y[0].re, 0.0};
  a[kBlock] = cd{Y[kBlock].re, 0.0};
  for (int k = 1; k < kBlock; k++) {
    a[k] = Y[k];
    a[kN - k] = cd{Y[k].re, -Y[k].im};
  }
  conv_ref::fft_radix2(a, kN, +1);
  for (int n = 0; n < kN; n++) y[n] = a[n].re / kN;
}
// the same two, term by term as the contract is written: O(N^2), for tests/rfft_ref_main.cpp
inline void rdft256_naive(const double* x, int len, cd* X) {
  const double pi = 3.14159265358979323846264338327950288;
  for (int k = 0; k < kBins; k++) {
    double re = 0.0, im = 0.0;
    for (int n = 0; n < len; n++) {
      const int ph = (k * n) % kN;   // (the angle reduced exactly)
      re += x[n] * std::cos(2.0 * pi * ph / kN);
      im -= x[n] * std::sin(2.0 * pi * ph / kN);
    }
    X[k] = cd{re, (k == 0 || k == kBlock) ? 0.0 : im};
  }
}
inline void inverse_naive(const cd* Y, double* y) {
  const double pi = 3.14159265358979323846264338327950288;
  for (int n = 0; n < kN; n++) {
    double acc = Y[0].re + ((n & 1) ? -Y[kBlock].re : Y[kBlock].re);
    for (int k = 1; k < kBlock; k++) {
      const int ph = (k * n) % kN;
      acc += 2.0 * (Y[k].re * std::cos(2.0 * pi * ph / kN) - Y[k].im * std::sin(2.0 * pi * ph / kN));
    }
    y[n] = acc / kN;
  }
}
// overlap-add of n inverse transforms y[t][0..256): out[t][0..128) = head_t + tail_{t-1}; overlap_in = tail_{-1}; overlap_out = tail_{n-1}
inline void overlap_add(const double* y, int n, const double* overlap_in, double* out, double* overlap_out) {
  for (int t = 0; t < n; t++)
    for (int i = 0; i < kBlock; i++) out[(size_t)t * kBlock + i] = y[(size_t)t * kN + i] + (t ? y[(size_t)(t - 1) * kN + kBlock + i] : overlap_in[i]);
  for (int i = 0; i < kBlock; i++) overlap_out[i] = y[(size_t)(n - 1) * kN + kBlock + i];
}

// ---- plane layouts: element (bin k, block t, row r) of planes with block extent T ------------------------------------------------------
inline size_t index_a(int k, int t, int r, int hist, int T, int rp) { return ((size_t)k * T + (size_t)(hist + t)) * rp + (size_t)r; }
inline size_t index_b(int r, int k, int t, int hist, int T) { return ((size_t)r * kBins + (size_t)k) * T + (size_t)(hist + t); }

}  // namespace rfft_ref
