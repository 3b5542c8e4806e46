// ga_ir_resample.hpp -- band-limited sample-rate conversion of an impulse response or an HRIR set (option "ir_resample", DESIGN.md
// section 8 "Impulse responses at another sample rate").  Host and device: the header compiles with plain g++ / clang++ as well as
// with hipcc.  The definition is this project's own (the reference refuses such a buffer, ConvolverNode.cs:22-23, 48-49); the truth
// is the float64 model tests/_ir_resample_model.py.
//
// Buffer rate fi, context rate fo, g = gcd(fi, fo), L = fo / g, D = fi / g.  rho = R min(1, fo / fi), W = ceil(Z / rho).
// N input frames give M = (N L + D - 1) / D output frames.  The interpolation kernel is a Kaiser-windowed sinc,
//   h(tau) = rho sinc(rho tau) I0(BETA sqrt(1 - v^2)) / I0(BETA),  v = rho tau / Z,  0 for |v| >= 1,
// and output m, with q, r = divmod(m D, L), is
//   y[m] = (fi / fo) sum over j = 0 .. 2W-1 of (double)x[q - W + 1 + j] tab[r][j],   tab[r][j] = h(r / L + W - 1 - j),
// terms outside the row skipped, j ascending, multiply and add separate double operations, one rounding to float at the end.  The
// factor fi / fo is there because the buffer is a filter, not a signal: the frequency response in Hz and the DC gain are kept.
//
// The table (L x 2W doubles) is made on the host (ir_resample_table: libm's sin and sqrt, I0 by its power series) and handed to
// whoever evaluates the sums, so that host and device run ir_resample_sample on the same numbers: identical bit patterns, provided
// no multiply-add pair is contracted (switched off below for the function's own body, as in ga_libmf.hpp).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GA_IRR_FN __host__ __device__ inline
#else
#define GA_IRR_FN inline
#endif

#if defined(__clang__)
#define GA_IRR_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define GA_IRR_NO_CONTRACT
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

namespace ga_irr {

constexpr int kZ = 64;            // zero crossings of the sinc on either side
constexpr double kBeta = 12.0;    // Kaiser window
constexpr double kR = 0.94;       // cut-off as a share of the lower Nyquist frequency
constexpr int64_t kMaxTable = (int64_t)1 << 22;   // L * 2W entries at most

struct Plan {
  int fi = 0, fo = 0;
  int64_t L = 0, D = 0;
  int W = 0;
  double rho = 0.0;
  double gain = 0.0;   // fi / fo
  int64_t entries() const { return L * 2 * (int64_t)W; }
};

// false: the rates are not positive, or the table would exceed kMaxTable entries
inline bool ir_resample_plan(int fi, int fo, Plan& p) {
  if (fi <= 0 || fo <= 0) return false;
  int64_t a = fi, b = fo;
  while (b) { const int64_t t = a % b; a = b; b = t; }
  p.fi = fi;
  p.fo = fo;
  p.L = fo / a;
  p.D = fi / a;
  const double ratio = (double)fo / (double)fi;
  p.rho = kR * (ratio < 1.0 ? ratio : 1.0);
  const double w = std::ceil((double)kZ / p.rho);
  p.gain = (double)fi / (double)fo;
  if (!(w >= 1.0) || w > (double)kMaxTable) return false;
  p.W = (int)w;
  return p.entries() <= kMaxTable;
}

// output frames of N input frames (N >= 0; N L stays far inside 64 bits for every buffer that fits a machine)
GA_IRR_FN int64_t ir_resample_length(int64_t N, int64_t L, int64_t D) { return (N * L + D - 1) / D; }

inline double ir_resample_i0(double x) {   // power series: sum ((x / 2)^2)^k / (k!)^2
  const double y = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; k++) {
    term *= y / ((double)k * (double)k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

inline double ir_resample_h(const Plan& p, double tau, double i0beta) {
  const double v = p.rho * tau / (double)kZ;
  if (!(std::fabs(v) < 1.0)) return 0.0;
  const double pi = 3.14159265358979323846264338327950288;
  const double u = p.rho * tau;
  const double s = u == 0.0 ? 1.0 : std::sin(pi * u) / (pi * u);
  return p.rho * s * ir_resample_i0(kBeta * std::sqrt(1.0 - v * v)) / i0beta;
}

// tab[r * 2W + j] = h(r / L + W - 1 - j)
inline std::vector<double> ir_resample_table(const Plan& p) {
  std::vector<double> tab((size_t)p.entries());
  const double i0beta = ir_resample_i0(kBeta);
  const int W2 = 2 * p.W;
  for (int64_t r = 0; r < p.L; r++)
    for (int j = 0; j < W2; j++) tab[(size_t)(r * W2 + j)] = ir_resample_h(p, (double)r / (double)p.L + (double)(p.W - 1 - j), i0beta);
  return tab;
}

// One output sample.  load(k) returns input frame k of the row, 0 <= k < N (a plain row on the host, the staged window on the
// device); row = tab + r * 2W.  This is the one place the sum is written down: the host program and the kernel both call it.
template <class Load>
GA_IRR_FN float ir_resample_sample(Load load, int64_t q, int64_t N, int W, const double* row, double gain) {
  GA_IRR_NO_CONTRACT
  const int64_t k0 = q - W + 1;
  const int64_t jlo = k0 < 0 ? -k0 : 0;
  const int64_t jhi = N - k0 < 2 * (int64_t)W ? N - k0 : 2 * (int64_t)W;
  double acc = 0.0;
  for (int64_t j = jlo; j < jhi; j++) {
    const double prod = (double)load(k0 + j) * row[j];
    acc = acc + prod;
  }
  return (float)(gain * acc);
}

// the whole row on the host: y[0 .. M), M = ir_resample_length(N, L, D)
inline void ir_resample_row(const float* x, int64_t N, const Plan& p, const double* tab, float* y) {
  const int64_t M = ir_resample_length(N, p.L, p.D);
  for (int64_t m = 0; m < M; m++) {
    const int64_t q = m * p.D / p.L, r = m * p.D % p.L;
    y[m] = ir_resample_sample([x](int64_t k) { return x[k]; }, q, N, p.W, tab + r * 2 * p.W, p.gain);
  }
}

}  // namespace ga_irr

#if !defined(__clang__)
#pragma GCC pop_options
#endif
