// The host arithmetic of the time-split biquad path (graphaudio_amd/csrc/ga_biquad_split.hpp) against tests/biquad_split_ref.hpp, and the
// reference against itself.  No GPU, no HIP: built with g++ under the address and undefined-behaviour sanitizers with
// -ffp-contract=off and run directly (tests/test_biquad_split_host.py).  One line per check, "check <name> ok|FAIL <figures>".
//
//   transition.*     A^K of the header (float64, repeated squaring) against K sequential steps of the recurrence in long double
//   split_equals_one_walk   where A^K is exactly zero the split model and the one walk give the same bits
//   deviation.*      the rounding-deviation predictor that mode 1 relies on, and what lies outside it
//   cut_rule         the pieces the planner cuts
//
// ---- the bound of `transition` ----------------------------------------------------------------------------------------------------
// Norms are 1-norms (largest column sum of magnitudes): submultiplicative, ||  |X|  || = ||X||, and no entry exceeds them.
// u = 2^-53 for the header, u' = 2^-64 for the reference; gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical
// Algorithms, Lemma 3.1).  N_m = ||A^m||, taken from the reference's own run: the state m steps after the unit state e_j IS column
// j of A^m.  Abar = the step matrix of the cascade with every coefficient replaced by its magnitude and every subtraction by an
// addition.  All bounds are to first order in u (products of two rounding errors are dropped, as in Higham's gamma calculus when
// bounds are chained): the terms dropped are smaller than the ones kept by the relative size of the bound itself, below 1e-6 here.
//
// One step of the recurrence evaluates, per section, w = v - a1 w1 - a2 w2 and o = b0 w + b1 w1 + b2 w2: at most 5 roundings
// between a section's input and its output, hence at most 5 nsec between a state entering the step and any value leaving it, and
// every intermediate is bounded in magnitude by the same expression over magnitudes.  So a computed step is
//   s^_{k+1} = A s^_k + d_k ,   |d_k| <= gamma_{5 nsec} Abar |s^_k|   componentwise                      (Higham, eq. 3.3 and Lemma 3.3)
// (a) the reference (K steps, long double): e_K = sum_m A^m d_{K-1-m}, hence
//       ||e_K|| <= gamma_{5 nsec}(u') ||Abar|| sum_{m=0}^{K-1} N_m N_{K-1-m}                                =: ref_bound
// (b) the header.  It holds A' = A^(2^i) and R = A^(K mod 2^i) when bit i is looked at; R <- R A' where the bit is set, then
//     A' <- A' A' while bits remain.  Every product P = fl(X Y) of D x D matrices has  |P - X Y| <= gamma_D(u) |X| |Y|  (eq. 3.13),
//     in norm  gamma_D N_a N_b  for X = A^a, Y = A^b.  What a local error does to the result:
//       - E in the A' of level i (the header's A itself for i = 0: ||E|| <= gamma_{5 nsec}(u) ||Abar||, one step from every unit
//         state; a squaring for i >= 1: ||E|| <= gamma_D N_{2^(i-1)}^2).  From there on the result is R A'^c with c = K >> i and
//         R = A^low, low = K mod 2^i, and  R (A' + E)^c - R A'^c = sum_{t<c} A^(low + 2^i t) E A^(2^i (c-1-t)):
//             contribution <= ||E|| sum_{t=0}^{c-1} N_{low + 2^i t} N_{2^i (c-1-t)}
//       - E in R <- R A' at bit i (||E|| <= gamma_D N_low N_{2^i}): what is still multiplied on is A^rest, rest = K - low - 2^i:
//             contribution <= ||E|| N_rest
//     eps_R = the sum of all contributions.
// (c) underflow: a product or sum below 2^-1022 is rounded on the subnormal grid, an absolute error of at most 2^-1075 that the
//     relative model does not cover; D of them per entry and D entries per column, carried on by norms that are below 1 wherever
//     something underflows: D^2 2^-1074 per product, (number of products) x that in all.
// The check asserts  max_ij |header - reference| <= eps_R + ref_bound + underflow.  The bound is a worst-case one: for a low cut-off
// N_m reaches 1 / sin(w0) (hundreds) before the poles' decay sets in, the sums above are of the order K N^2, and the error that is
// observed is a few per cent of the bound at most (the largest observed / bound ratio is printed, with the largest observed error
// relative to the largest entry of A^K: repeated squaring doubles a relative error per squaring, and at K = 16,384 the float64
// result is off by up to ~1e-7 of the largest entry -- of entries that are then ~1e-17, against pass A states of order 1).
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ga_biquad_split.hpp"
#include "biquad_split_ref.hpp"

namespace br = bq_ref;

static int failures = 0;
static void check(const std::string& name, bool ok, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  std::printf("check %s %s %s\n", name.c_str(), ok ? "ok" : "FAIL", buf);
  std::fflush(stdout);
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
  double unit() { return ((double)(next() >> 11) + 0.5) / 9007199254740992.0; }   // (0, 1)
  double gauss() { return std::sqrt(-2.0 * std::log(unit())) * std::cos(6.283185307179586 * unit()); }
};
static std::vector<float> white(Rng& r, int64_t n) {   // unit variance
  std::vector<float> x((size_t)n);
  for (auto& v : x) v = (float)r.gauss();
  return x;
}
static std::vector<float> coefs_of(const std::vector<br::Sec>& s) {
  std::vector<float> c;
  for (const br::Sec& q : s) c.insert(c.end(), {q.b0, q.b1, q.b2, q.a1, q.a2});
  return c;
}
static double rms_diff(const float* a, const float* b, int64_t n) {
  double s = 0;
  for (int64_t i = 0; i < n; i++) s += ((double)a[i] - b[i]) * ((double)a[i] - b[i]);
  return std::sqrt(s / (double)n);
}
static double rms_diff(const float* a, const double* b, int64_t n) {
  double s = 0;
  for (int64_t i = 0; i < n; i++) s += ((double)a[i] - b[i]) * ((double)a[i] - b[i]);
  return std::sqrt(s / (double)n);
}

// the HARD list of tests/test_gpu_biquad_split.py, then mid-band filters
static const struct { br::Type t; double f, q, g; } kFilters[] = {
    {br::kLowpass, 40.0, 0.707, 0.0},   {br::kLowpass, 200.0, 10.0, 0.0},  {br::kHighpass, 30.0, 0.707, 0.0},   {br::kHighpass, 80.0, 10.0, 0.0},
    {br::kBandpass, 60.0, 8.0, 0.0},    {br::kNotch, 50.0, 10.0, 0.0},     {br::kPeaking, 100.0, 10.0, 12.0},   {br::kLowshelf, 60.0, 1.0, -12.0},
    {br::kHighshelf, 12000.0, 1.0, 9.0}, {br::kAllpass, 300.0, 5.0, 0.0},
    {br::kPeaking, 1500.0, 1.0, 5.0},   {br::kPeaking, 5000.0, 1.0, 5.0},  {br::kLowpass, 3000.0, 0.707, 0.0},  {br::kHighpass, 2000.0, 1.0, 0.0},
    {br::kBandpass, 4000.0, 2.0, 0.0},  {br::kNotch, 7000.0, 1.5, 0.0},    {br::kLowshelf, 2500.0, 0.8, 4.0},   {br::kAllpass, 9000.0, 0.9, 0.0},
};
constexpr int kNumHard = 10, kNumFilters = (int)(sizeof kFilters / sizeof kFilters[0]);
static br::Sec filter(int i) { return br::rbj(kFilters[i].t, kFilters[i].f, kFilters[i].q, kFilters[i].g); }

static long double gamma_n(int n, long double u) { return n * u / (1.0L - n * u); }

static void transition_checks() {
  const int64_t Ks[] = {1, 2, 3, 32, 768, 1024, 1056, 16384};
  const long double u = std::ldexp(1.0L, -53), ul = std::ldexp(1.0L, -64);
  double worst_ratio = 0, worst_rel = 0;
  for (int nsec = 1; nsec <= 8; nsec++) {
    // three cascades per length: hard filters only, mid-band only, both alternating (every filter of the list is used)
    for (int variant = 0; variant < 3; variant++) {
      std::vector<br::Sec> secs;
      for (int q = 0; q < nsec; q++) {
        int i = variant == 0 ? (nsec + q) % kNumHard : variant == 1 ? kNumHard + (nsec + q) % (kNumFilters - kNumHard) : (2 * nsec + 5 * q) % kNumFilters;
        secs.push_back(filter(i));
      }
      const std::vector<float> coefs = coefs_of(secs);
      const int D = 2 * nsec;
      // ||Abar||: one step of the magnitude cascade from every unit state
      long double nabar = 0;
      for (int j = 0; j < D; j++) {
        std::vector<long double> st(D, 0.0L);
        st[j] = 1.0L;
        long double v = 0, sum = 0;
        for (int q = 0; q < nsec; q++) {
          const long double w1 = st[2 * q], w2 = st[2 * q + 1];
          const long double w = v + std::fabs((long double)secs[q].a1) * w1 + std::fabs((long double)secs[q].a2) * w2;
          v = std::fabs((long double)secs[q].b0) * w + std::fabs((long double)secs[q].b1) * w1 + std::fabs((long double)secs[q].b2) * w2;
          st[2 * q + 1] = w1;
          st[2 * q] = w;
        }
        for (int r = 0; r < D; r++) sum += st[r];
        nabar = std::max(nabar, sum);
      }
      bool ok = true;
      double case_ratio = 0, case_rel = 0;
      for (int64_t K : Ks) {
        std::vector<long double> N;
        const std::vector<long double> ref = br::transition_seq(secs.data(), nsec, K, &N);
        long double conv = 0;
        for (int64_t m = 0; m < K; m++) conv += N[(size_t)m] * N[(size_t)(K - 1 - m)];
        const long double ref_bound = gamma_n(5 * nsec, ul) * nabar * conv;
        // the header's multiplication order
        auto S = [&](int i, int64_t low, int64_t c) {
          long double sum = 0;
          for (int64_t t = 0; t < c; t++) sum += N[(size_t)(low + (t << i))] * N[(size_t)((c - 1 - t) << i)];
          return sum;
        };
        long double epsR = gamma_n(5 * nsec, u) * nabar * S(0, 0, K);
        int products = 0;
        for (int i = 0; (K >> i) > 0; i++) {
          const int64_t low = K & (((int64_t)1 << i) - 1), p = (int64_t)1 << i;
          if ((K >> i) & 1) {
            epsR += gamma_n(D, u) * N[(size_t)low] * N[(size_t)p] * N[(size_t)(K - low - p)];
            products++;
          }
          if ((K >> i) > 1) {
            epsR += gamma_n(D, u) * N[(size_t)p] * N[(size_t)p] * S(i + 1, K & (2 * p - 1), K >> (i + 1));
            products++;
          }
        }
        const long double underflow = products * (long double)D * D * std::ldexp(1.0L, -1074);
        const std::vector<double> got = ga::biquad_split_transition(coefs.data(), nsec, K);
        long double err = 0, big = 0;
        for (size_t i = 0; i < got.size(); i++) {
          err = std::max(err, std::fabs((long double)got[i] - ref[i]));
          big = std::max(big, std::fabs(ref[i]));
        }
        const long double bound = epsR + ref_bound + underflow;
        ok = ok && err <= bound && got.size() == (size_t)D * D;
        if (bound > 0) case_ratio = std::max(case_ratio, (double)(err / bound));
        if (big > std::ldexp(1.0L, -900)) case_rel = std::max(case_rel, (double)(err / big));
      }
      worst_ratio = std::max(worst_ratio, case_ratio);
      worst_rel = std::max(worst_rel, case_rel);
      const char* vn = variant == 0 ? "hard" : variant == 1 ? "mid" : "mixed";
      check("transition.s" + std::to_string(nsec) + "." + vn, ok, "largest observed/bound %.3g, largest observed/max|A^K| %.3g", case_ratio, case_rel);
    }
  }
  std::printf("transition: largest observed/bound %.3g, largest observed/max|A^K| %.3g\n", worst_ratio, worst_rel);
}

// Where A^K is exactly zero the scan hands piece l the end state of piece l - 1's walk from ZERO; the one walk hands it the end state
// of the walk from the true state.  Both walks see the same K inputs, and the difference of their states is multiplied by A every
// step while it is representable: once it has fallen below the states' spacing the two walks are the same bits and stay so.
static void split_equals_one_walk() {
  Rng rng{0x5EED0001};
  bool ok = true;
  double maxM = 0;
  int64_t first_bad = -1;
  const int64_t K = 16384;   // (pole radii up to 0.92: 0.92^16384 is below the smallest float64 subnormal, A^K underflows to exactly zero)
  const int G = 3;
  const int64_t n = (G - 1) * K + 1056;
  for (int nsec = 1; nsec <= 8 && ok; nsec++) {
    std::vector<br::Sec> secs;
    for (int q = 0; q < nsec; q++) secs.push_back(filter(kNumHard + (3 * nsec + q) % (kNumFilters - kNumHard)));
    const std::vector<double> M = ga::biquad_split_transition(coefs_of(secs).data(), nsec, K);
    for (double v : M) maxM = std::max(maxM, std::fabs(v));
    const std::vector<float> x = white(rng, n);
    const int D = 2 * nsec;
    std::vector<float> s0(D), one_state, y1((size_t)n), y2((size_t)n, -77.f), scratch((size_t)(G - 1) * D, 0.f);
    for (auto& v : s0) v = (float)rng.gauss();
    one_state = s0;
    br::walk_f32(secs.data(), nsec, x.data(), y1.data(), n, one_state.data());
    std::vector<float> st = s0;
    br::split_f32(secs.data(), nsec, M.data(), x.data(), y2.data(), n, G, K, 1, st.data(), scratch.data());
    // piece 0 starts from s_0 in both; from piece 1 on the split starts from the zero-state walk's end state
    for (int64_t i = 0; i < n && ok; i++)
      if (std::memcmp(&y1[(size_t)i], &y2[(size_t)i], 4) != 0) {
        ok = false;
        first_bad = i;
      }
    ok = ok && std::memcmp(one_state.data(), st.data(), (size_t)D * 4) == 0;
  }
  check("split_equals_one_walk", ok && maxM == 0.0, "1..8 mid-band sections, K %lld, G %d: max|A^K| %g, first differing frame %lld", (long long)K, G,
        maxM, (long long)first_bad);
}

struct Measured {
  double predicted, split_vs_one, one_vs_f64, split_vs_f64;
};
// K = 768 in 256 pieces, the most the planner cuts: 196,608 frames of white input of unit variance from the zero state.  The predictor
// speaks of an RMS over stationary input, so the measurement has to average over many time constants of the slowest pole of the
// sweep below (Q 10 at 20 Hz: Q sr / (pi f) = 7,640 frames): 25 of them here.
static Measured measure(const std::vector<br::Sec>& secs, Rng& rng) {
  const int nsec = (int)secs.size(), D = 2 * nsec;
  const int64_t K = 768;
  const int G = 256;
  const int64_t n = K * G;
  const std::vector<float> c = coefs_of(secs);
  Measured m;
  m.predicted = ga::biquad_split_deviation(c.data(), nsec);
  const std::vector<double> M = ga::biquad_split_transition(c.data(), nsec, K);
  const std::vector<float> x = white(rng, n);
  std::vector<float> y1((size_t)n), y2((size_t)n), st1(D, 0.f), st2(D, 0.f), scratch((size_t)(G - 1) * D, 0.f);
  std::vector<double> y64((size_t)n), st64(D, 0.0);
  br::walk_f32(secs.data(), nsec, x.data(), y1.data(), n, st1.data());
  br::split_f32(secs.data(), nsec, M.data(), x.data(), y2.data(), n, G, K, 1, st2.data(), scratch.data());
  br::walk_f64(secs.data(), nsec, x.data(), y64.data(), n, st64.data());
  m.split_vs_one = rms_diff(y2.data(), y1.data(), n);
  m.one_vs_f64 = rms_diff(y1.data(), y64.data(), n);
  m.split_vs_f64 = rms_diff(y2.data(), y64.data(), n);
  return m;
}

// The pinned figure: the worst (split's error against float64) / (one walk's error against float64) over the sweep below, measured on
// the CPU with this seed, and what the check allows (1.25 x it).  The model is deterministic: a pin, not a tolerance.
constexpr double kWorstErrorRatioMeasured = 1.0892;
constexpr double kErrorRatioAllowed = 1.25 * kWorstErrorRatioMeasured;
constexpr double kSplitMaxDeviation = 2.5e-6;   // the default of option biquad_split_max_deviation

static void deviation_checks() {
  Rng rng{0xB1C0AD5EEDull};
  const int want = 270;
  int have = 0, drawn = 0;
  double worst_pred = 0, worst_err = 0, worst_abs = 0;
  bool ok_pred = true, ok_err = true;
  std::string over;   // the cascades whose measured deviation exceeds the predicted one
  while (have < want && drawn < 20000) {
    drawn++;
    const int nsec = 1 + (int)(rng.next() % 3);
    std::vector<br::Sec> secs;
    for (int q = 0; q < nsec; q++) {
      const br::Type t = (br::Type)(rng.next() % 8);
      const double f = 20.0 * std::pow(1000.0, rng.unit());   // 20 Hz .. 20 kHz
      const double Q = 0.3 * std::pow(10.0 / 0.3, rng.unit());
      const double g = -12.0 + 24.0 * rng.unit();
      secs.push_back(br::rbj(t, f, Q, g));
    }
    if (ga::biquad_split_deviation(coefs_of(secs).data(), nsec) > kSplitMaxDeviation) continue;
    have++;
    const Measured m = measure(secs, rng);
    worst_pred = std::max(worst_pred, m.split_vs_one / m.predicted);
    ok_pred = ok_pred && m.split_vs_one <= m.predicted;
    worst_abs = std::max(worst_abs, m.split_vs_one);
    if (m.split_vs_one > m.predicted) {
      char buf[256];
      std::snprintf(buf, sizeof buf, " | cascade %d: predicted %.3g measured %.3g, a1 a2 =", have, m.predicted, m.split_vs_one);
      over += buf;
      for (const br::Sec& q : secs) {
        std::snprintf(buf, sizeof buf, " (%.6g %.6g)", q.a1, q.a2);
        over += buf;
      }
    }
    if (m.one_vs_f64 > 0) worst_err = std::max(worst_err, m.split_vs_f64 / m.one_vs_f64);
    ok_err = ok_err && m.split_vs_f64 <= kErrorRatioAllowed * m.one_vs_f64;
  }
  check("deviation.predictor_bounds_the_split", ok_pred && have == want, "%d cascades of 1-3 sections inside %.2g (of %d drawn): worst measured/predicted %.3f%s",
        have, kSplitMaxDeviation, drawn, worst_pred, over.substr(0, 300).c_str());
  // (what mode 1 promises the user: a cascade it splits deviates from the one walk by less than the option's value)
  check("deviation.split_cascades_stay_inside_the_option", worst_abs <= kSplitMaxDeviation && have == want, "largest measured %.3g, option %.3g", worst_abs,
        kSplitMaxDeviation);
  check("deviation.split_as_close_to_float64_as_one_walk", ok_err && have == want, "worst (split - f64) / (one walk - f64) %.4f, pinned %.4f, allowed %.4f",
        worst_err, kWorstErrorRatioMeasured, kErrorRatioAllowed);
  // outside the threshold (reached only with biquad_time_split = 2): the prediction is no upper bound there, and the split is further
  // from float64 than the one walk.  Figures are printed; asserted is only that mode 1 declines these cascades.
  struct Out { const char* name; std::vector<br::Sec> secs; };
  const Out outs[] = {
      {"lowpass_45.7Hz_Q3.95", {br::rbj(br::kLowpass, 45.7, 3.95, 0)}},
      {"allpass_21Hz_Q1.2_in_3_sections", {br::rbj(br::kPeaking, 1500.0, 1.0, 5.0), br::rbj(br::kAllpass, 21.0, 1.2, 0), br::rbj(br::kPeaking, 5000.0, 1.0, 5.0)}},
      {"lowpass_20Hz_Q0.5", {br::rbj(br::kLowpass, 20.0, 0.5, 0)}},
  };
  for (const Out& o : outs) {
    const Measured m = measure(o.secs, rng);
    check(std::string("deviation.mode1_declines.") + o.name, m.predicted > kSplitMaxDeviation,
          "predicted %.3g, measured split-vs-one-walk %.3g (x%.2f), one walk vs f64 %.3g, split vs f64 %.3g (x%.2f)", m.predicted, m.split_vs_one,
          m.split_vs_one / m.predicted, m.one_vs_f64, m.split_vs_f64, m.split_vs_f64 / m.one_vs_f64);
  }
}

static void cut_rule() {
  // cascade heads on a level: config 2 (256 and 1024 voices, one low-pass each), config 4 (64 .. 8192 voices x 5 sections: one head
  // per voice), and 1 and 65536 for the ends of the rule
  const int heads[] = {1, 64, 256, 1024, 4096, 8192, 65536};
  bool ok = true;
  int split = 0, maxG = 0;
  long long bad_m = -1;
  for (int h : heads)
    for (int64_t m = 1; m <= 12000 && ok; m += (m < 1200 ? 1 : 7)) {
      const int64_t nf = 128 * m;
      const ga::BiquadSplitCut c = ga::biquad_split_cut(nf, h);
      bool good = c.G >= 1 && c.G <= 256;
      if (c.G == 1) good = good && c.K == nf;
      else {
        split++;
        good = good && c.K % 32 == 0 && c.K >= 32;
        good = good && (int64_t)(c.G - 1) * c.K < nf && nf <= (int64_t)c.G * c.K;   // the pieces tile [0, nf), the last one not empty
        good = good && (nf - (int64_t)(c.G - 1) * c.K) % 32 == 0;
      }
      maxG = std::max(maxG, c.G);
      if (!good) {
        ok = false;
        bad_m = m;
      }
    }
  check("cut_rule", ok && split > 0 && maxG == 256, "%d cuts with G > 1, largest G %d, first bad nf / 128 = %lld", split, maxG, bad_m);
}

int main() {
  transition_checks();
  split_equals_one_walk();
  deviation_checks();
  cut_rule();
  std::printf("%s\n", failures ? "FAILED" : "all ok");
  return failures ? 1 : 0;
}
