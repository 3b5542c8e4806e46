// The contracts of the time-split biquad path (graphaudio_amd/csrc/ga_kernels.hpp, BiquadScanJob) in plain C++: no HIP, nothing taken
// from the product's headers.  Build with -ffp-contract=off and without fast-math or flush-to-zero: every float operation below is
// meant to round once, exactly as written.
//   walk_f32     the float32 recurrence, one section after the other, operations as in BiQuadFilterNode.cs:137-138
//   walk_f64     the same recurrence in float64 on the float coefficients
//   scan         s_{l+1} = (float)(z_l + sum_c M[r][c] s_l[c]), M and the accumulation in float64, c ascending, two float roundings
//   split_f32    pass A from the zero state, the scan, pass B, twins
//   expand       the pieces of a cascade as job records
//   transition_seq  A^K by K sequential steps of the recurrence from the unit states, long double
//   rbj          test filters (the RBJ cookbook in float64, rounded to float: the checks do not need the product's own coefficients)
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace bq_ref {

struct Sec {
  float b0, b1, b2, a1, a2;
};
enum Type { kLowpass, kHighpass, kBandpass, kNotch, kAllpass, kPeaking, kLowshelf, kHighshelf };

inline Sec rbj(Type t, double f, double q, double gain_db, double sr = 48000.0) {
  const double w0 = 2.0 * 3.14159265358979323846 * f / sr, c = std::cos(w0), s = std::sin(w0), al = s / (2.0 * q);
  const double A = std::pow(10.0, gain_db / 40.0), be = std::sqrt(A) / q;
  double b0 = 1, b1 = 0, b2 = 0, a0 = 1, a1 = 0, a2 = 0;
  switch (t) {
    case kLowpass: b0 = (1 - c) / 2; b1 = 1 - c; b2 = (1 - c) / 2; a0 = 1 + al; a1 = -2 * c; a2 = 1 - al; break;
    case kHighpass: b0 = (1 + c) / 2; b1 = -(1 + c); b2 = (1 + c) / 2; a0 = 1 + al; a1 = -2 * c; a2 = 1 - al; break;
    case kBandpass: b0 = al; b1 = 0; b2 = -al; a0 = 1 + al; a1 = -2 * c; a2 = 1 - al; break;
    case kNotch: b0 = 1; b1 = -2 * c; b2 = 1; a0 = 1 + al; a1 = -2 * c; a2 = 1 - al; break;
    case kAllpass: b0 = 1 - al; b1 = -2 * c; b2 = 1 + al; a0 = 1 + al; a1 = -2 * c; a2 = 1 - al; break;
    case kPeaking: b0 = 1 + al * A; b1 = -2 * c; b2 = 1 - al * A; a0 = 1 + al / A; a1 = -2 * c; a2 = 1 - al / A; break;
    case kLowshelf:
      b0 = A * ((A + 1) - (A - 1) * c + be * s); b1 = 2 * A * ((A - 1) - (A + 1) * c); b2 = A * ((A + 1) - (A - 1) * c - be * s);
      a0 = (A + 1) + (A - 1) * c + be * s; a1 = -2 * ((A - 1) + (A + 1) * c); a2 = (A + 1) + (A - 1) * c - be * s;
      break;
    case kHighshelf:
      b0 = A * ((A + 1) + (A - 1) * c + be * s); b1 = -2 * A * ((A - 1) + (A + 1) * c); b2 = A * ((A + 1) + (A - 1) * c - be * s);
      a0 = (A + 1) - (A - 1) * c + be * s; a1 = 2 * ((A - 1) - (A + 1) * c); a2 = (A + 1) - (A - 1) * c - be * s;
      break;
  }
  return Sec{(float)(b0 / a0), (float)(b1 / a0), (float)(b2 / a0), (float)(a1 / a0), (float)(a2 / a0)};
}

// state: [nsec][2] = {W1, W2} of every section, in and out.  y may be nullptr (the state is advanced, nothing is written).
inline void walk_f32(const Sec* s, int nsec, const float* x, float* y, int64_t n, float* state) {
  for (int64_t i = 0; i < n; i++) {
    float v = x[i];
    for (int q = 0; q < nsec; q++) {
      float& w1 = state[2 * q];
      float& w2 = state[2 * q + 1];
      const float w = v - s[q].a1 * w1 - s[q].a2 * w2;           // BiQuadFilterNode.cs:137
      const float o = s[q].b0 * w + s[q].b1 * w1 + s[q].b2 * w2;   // :138
      w2 = w1;
      w1 = w;
      v = o;
    }
    if (y) y[i] = v;
  }
}
inline void walk_f64(const Sec* s, int nsec, const float* x, double* y, int64_t n, double* state) {
  for (int64_t i = 0; i < n; i++) {
    double v = x[i];
    for (int q = 0; q < nsec; q++) {
      double& w1 = state[2 * q];
      double& w2 = state[2 * q + 1];
      const double w = v - (double)s[q].a1 * w1 - (double)s[q].a2 * w2;
      const double o = (double)s[q].b0 * w + (double)s[q].b1 * w1 + (double)s[q].b2 * w2;
      w2 = w1;
      w1 = w;
      v = o;
    }
    if (y) y[i] = v;
  }
}

// A^K, row-major [D][D], D = 2 nsec: column j is the state K steps after the unit state e_j with zero input.
// colsum_max, if given, receives ||A^m||_1 for m = 0 .. K: the largest column sum of magnitudes (the state after m steps IS a column of A^m).
inline std::vector<long double> transition_seq(const Sec* s, int nsec, int64_t K, std::vector<long double>* colsum_max = nullptr) {
  const int D = 2 * nsec;
  std::vector<long double> R((size_t)D * D, 0.0L);
  if (colsum_max) colsum_max->assign((size_t)K + 1, 0.0L);
  for (int j = 0; j < D; j++) {
    std::vector<long double> st(D, 0.0L);
    st[j] = 1.0L;
    for (int64_t k = 0; k <= K; k++) {
      if (colsum_max) {
        long double sum = 0;
        for (int r = 0; r < D; r++) sum += std::fabs(st[r]);
        if (sum > (*colsum_max)[(size_t)k]) (*colsum_max)[(size_t)k] = sum;
      }
      if (k == K) break;
      long double v = 0.0L;
      for (int q = 0; q < nsec; q++) {
        long double& w1 = st[2 * q];
        long double& w2 = st[2 * q + 1];
        const long double w = v - (long double)s[q].a1 * w1 - (long double)s[q].a2 * w2;
        const long double o = (long double)s[q].b0 * w + (long double)s[q].b1 * w1 + (long double)s[q].b2 * w2;
        w2 = w1;
        w1 = w;
        v = o;
      }
    }
    for (int r = 0; r < D; r++) R[(size_t)r * D + j] = st[r];
  }
  return R;
}

// The scan.  scratch: [G - 1][D], in: z_l of pass A, out: s_l, where pass B's piece l starts.  state: [D], in: s_0, out: s_{G-1}.
inline void scan(const double* M, int D, int G, float* scratch, float* state) {
  std::vector<double> cur(D), nxt(D);
  for (int r = 0; r < D; r++) cur[r] = (double)state[r];
  for (int l = 0; l + 1 < G; l++) {
    float* sc = scratch + (size_t)l * D;
    for (int r = 0; r < D; r++) {
      double a = (double)sc[r];
      for (int c = 0; c < D; c++) a += M[r * D + c] * cur[c];
      nxt[r] = a;
    }
    for (int r = 0; r < D; r++) {
      sc[r] = (float)cur[r];
      cur[r] = (double)(float)nxt[r];
    }
  }
  for (int r = 0; r < D; r++) state[r] = (float)cur[r];
}

// One piece of a cascade cut into G pieces of K frames: what the expanded job tables hold.
struct Piece {
  int64_t f0, n;        // first frame (relative to the views), frames
  int64_t state_off;    // floats into the cascade's scratch; -1: the sections' own state (the last piece)
  int twins;
  bool out;             // false: the job only advances its state (pass A)
};
inline void expand(int64_t f0, int64_t n, int nsec, int twins, int G, int64_t K, std::vector<Piece>& passA, std::vector<Piece>& passB) {
  for (int l = 0; l < G; l++) {
    Piece p;
    p.f0 = f0 + (int64_t)l * K;
    p.n = n - (int64_t)l * K < K ? n - (int64_t)l * K : K;
    p.state_off = l + 1 < G ? (int64_t)l * nsec * 2 : -1;
    p.twins = l + 1 < G ? 1 : twins;
    p.out = true;
    passB.push_back(p);
    if (l + 1 < G) {
      p.out = false;
      p.twins = 1;
      passA.push_back(p);
    }
  }
}

// The split evaluation of one cascade over x[0, n).  state: the persistent state, [nsec][twins][2] (the twin channels of a section
// side by side: section q's own slot is state + 2 twins q, twin t's at + 2 t); in: s_0 from twin 0, out: the end state in every
// twin's slot.  scratch: [G - 1][nsec][2], left as the kernels leave it (pieces 0 .. G-2 end states after pass B).
inline void split_f32(const Sec* s, int nsec, const double* M, const float* x, float* y, int64_t n, int G, int64_t K, int twins, float* state,
                      float* scratch) {
  const int D = 2 * nsec;
  std::vector<Piece> pa, pb;
  expand(0, n, nsec, twins, G, K, pa, pb);
  for (const Piece& p : pa) {   // pass A: from the zero state (the caller's scratch is zero), outputs dropped
    float* st = scratch + p.state_off;
    for (int r = 0; r < D; r++) st[r] = 0.f;
    walk_f32(s, nsec, x + p.f0, nullptr, p.n, st);
  }
  std::vector<float> own(D);
  for (int q = 0; q < nsec; q++) {
    own[2 * q] = state[2 * twins * q];
    own[2 * q + 1] = state[2 * twins * q + 1];
  }
  scan(M, D, G, scratch, own.data());
  for (const Piece& p : pb) walk_f32(s, nsec, x + p.f0, y + p.f0, p.n, p.state_off >= 0 ? scratch + p.state_off : own.data());
  for (int q = 0; q < nsec; q++)
    for (int t = 0; t < twins; t++) {
      state[2 * twins * q + 2 * t] = own[2 * q];
      state[2 * twins * q + 2 * t + 1] = own[2 * q + 1];
    }
}

}  // namespace bq_ref
