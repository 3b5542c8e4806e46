// ga_biquad_split.hpp -- the host arithmetic of constant-coefficient biquad cascades split along time (ga_kernels.hpp,
// BiquadScanJob): the rounding-deviation model that decides in mode 1 which cascades may be split, the transition matrix A and
// its power A^K that the scan kernels multiply with, and the rule that cuts a segment into pieces.  Host-only, no HIP and no
// caches: Context (ga_engine.cpp, ga_plan_nodes.cpp) remembers the results per coefficient set; tests/biquad_split_main.cpp
// calls the functions directly.  coefs: [nsec][5] = b0 b1 b2 a1 a2 of every section.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ga {

// Predicted RMS difference between two float32 evaluations of a cascade that round differently, for white input of unit variance.
inline double biquad_split_deviation(const float* coefs, int nsec) {
  // Rounding-noise model (white input): the rounding of section q's  w = x - a1 w1 - a2 w2  is an error of ~ 2^-24 / sqrt(3) |w|
  // entering at that section's input; it reaches the output through sections q .. nsec-1.  With g_q = energy of the impulse response
  // input -> w_q and t_q = energy of (input of section q -> output), the noise-to-signal ratio is eps^2 sum_q g_q t_q / energy of the
  // whole cascade; two evaluations that round differently differ by sqrt(2) of that.
  const int N = 1 << 14;
  std::vector<double> sig(N, 0.0);
  sig[0] = 1.0;
  std::vector<std::vector<double>> wq(nsec);
  for (int q = 0; q < nsec; q++) {   // impulse response of the first q sections + 1/A_q: the W of section q
    const double b0 = coefs[5 * q], b1 = coefs[5 * q + 1], b2 = coefs[5 * q + 2], a1 = coefs[5 * q + 3], a2 = coefs[5 * q + 4];
    wq[q].resize(N);
    double w1 = 0, w2 = 0;
    for (int i = 0; i < N; i++) {
      const double w = sig[i] - a1 * w1 - a2 * w2;
      wq[q][i] = w;
      sig[i] = b0 * w + b1 * w1 + b2 * w2;
      w2 = w1;
      w1 = w;
    }
  }
  double acc = 0;
  for (int q = 0; q < nsec; q++) {
    std::vector<double> tail(N, 0.0);
    tail[0] = 1.0;
    for (int r = q; r < nsec; r++) {
      const double b0 = coefs[5 * r], b1 = coefs[5 * r + 1], b2 = coefs[5 * r + 2], a1 = coefs[5 * r + 3], a2 = coefs[5 * r + 4];
      double w1 = 0, w2 = 0;
      for (int i = 0; i < N; i++) {
        const double w = tail[i] - a1 * w1 - a2 * w2;
        tail[i] = b0 * w + b1 * w1 + b2 * w2;
        w2 = w1;
        w1 = w;
      }
    }
    double g = 0, tt = 0;
    for (int i = 0; i < N; i++) {
      g += wq[q][i] * wq[q][i];
      tt += tail[i] * tail[i];
    }
    acc += g * tt;
  }
  const double eps = 5.96e-8 / 1.7320508;
  // absolute, for white input of unit variance; x 3: what the measured deviations are above this model (tests/test_gpu_biquad_split.py)
  return 3.0 * std::sqrt(2.0 * eps * eps * acc);
}

// A of a cascade's state recursion (state = W1, W2 of every section, direct form II as in BiQuadFilterNode.cs:137-141), float64,
// row-major [2 nsec][2 nsec]: one step from the unit states with zero input gives the columns of A
inline std::vector<double> biquad_split_step_matrix(const float* coefs, int nsec) {
  const int D = 2 * nsec;
  std::vector<double> A((size_t)D * D, 0.0);
  for (int j = 0; j < D; j++) {
    std::vector<double> st(D, 0.0);
    st[j] = 1.0;
    double x = 0.0;
    for (int q = 0; q < nsec; q++) {
      const double b0 = coefs[5 * q], b1 = coefs[5 * q + 1], b2 = coefs[5 * q + 2], a1 = coefs[5 * q + 3], a2 = coefs[5 * q + 4];
      const double w1 = st[2 * q], w2 = st[2 * q + 1];
      const double w = x - a1 * w1 - a2 * w2;
      x = b0 * w + b1 * w1 + b2 * w2;
      st[2 * q + 1] = w1;
      st[2 * q] = w;
    }
    for (int r = 0; r < D; r++) A[(size_t)r * D + j] = st[r];
  }
  return A;
}

// A^K by repeated squaring (the bits of K from the lowest: R <- R A where the bit is set, A <- A A while bits remain), row-major
// [2 nsec][2 nsec].  The scan kernels read it as float64: for a low cut-off the entries of A^K and the states W1, W2 are both of the
// order 1 / sin(w0) (hundreds) and  A^K s  cancels down to that order again, so a matrix rounded to float puts 2^-24 x 10^4..10^5 into
// every handed-over state -- measured (tests/biquad_split_main.cpp, deviation.*): up to twice the one walk's distance from float64
// and 1.22 x the deviation that biquad_split_deviation predicts, against 1.13 x and 0.86 x with float64 entries.
inline std::vector<double> biquad_split_transition(const float* coefs, int nsec, int64_t K) {
  const int D = 2 * nsec;
  std::vector<double> A = biquad_split_step_matrix(coefs, nsec), R((size_t)D * D, 0.0), T((size_t)D * D);
  for (int i = 0; i < D; i++) R[(size_t)i * D + i] = 1.0;
  auto mul = [&](std::vector<double>& out, const std::vector<double>& a, const std::vector<double>& b) {
    for (int i = 0; i < D; i++)
      for (int j = 0; j < D; j++) {
        double acc = 0.0;
        for (int k = 0; k < D; k++) acc += a[(size_t)i * D + k] * b[(size_t)k * D + j];
        T[(size_t)i * D + j] = acc;
      }
    out = T;
  };
  for (int64_t e = K; e > 0; e >>= 1) {
    if (e & 1) mul(R, R, A);
    if (e > 1) mul(A, A, A);
  }
  return R;
}

// The cut of a segment of nf frames into G pieces of K frames (the last one shorter): as many pieces as keep every lane of the chip
// busy with `heads` cascade heads on the level, each >= 1024 frames, at most 256; K is rounded up to whole cache lines per piece
// (biquad1_kernel reads 128 bytes per round) and G recomputed.  G = 1: one walk, K = nf.
struct BiquadSplitCut {
  int G;
  int64_t K;
};
inline BiquadSplitCut biquad_split_cut(int64_t nf, int heads) {
  const int64_t lanes = 64 * 1024, h = std::max(heads, 1);
  int G = (int)std::max<int64_t>(1, std::min<int64_t>({(lanes + h - 1) / h, nf / 1024, 256}));
  const int64_t K = G > 1 ? ((nf + G - 1) / G + 31) / 32 * 32 : nf;
  if (G > 1) G = (int)((nf + K - 1) / K);
  return BiquadSplitCut{G, K};
}

}  // namespace ga
