// Stand-alone run of the seven 256-point real-FFT kernel instances of graphaudio_amd/csrc/ga_rfft.hip through their launchers alone,
// against the float64 reference tests/rfft_ref.hpp.  (tests/rfft_kernels_main.hip pins the same kernels' bits with recorded digests;
// this program is what says the bits are right.)  argv[1] picks a family:
//   fwd    rfft_fwd_kernel (A), rfft_fwd_b_kernel<float> (b32) and <double> (b64) on the same signals, against the float64 DFT
//   inv    irfft_ola_kernel (A), irfft_ola_b_kernel<float|double> on the same spectra, two chunks chained through the overlap
//   exact  bit-for-bit identities that need no reference: equal blocks give equal columns, equal columns give equal blocks (the
//          33rd transform of a full run, alone on one wave, against the batched ones), one chunk against the same blocks in two
//   seam   65,537 rows / jobs through the three launchers that cut their grid at 65,535: every row has row 0's bits
//   chain  forward -> partition sum -> inverse on the device against direct float64 convolution, B (float and double) and A
// Every output array lies between two guard regions filled with the byte 0xCD like the array itself: the guards must be untouched,
// every element the contract says is written must be right, every other element must still read 0xCD.  Input arrays lie between guard
// regions of NaN and every input element the contract says is not read is NaN (the samples behind a row's last block, the spectra from
// block `nblocks` on, formulation A's rows from `nrows` on): one NaN in a checked output means a read outside the contract.  Before a
// launch the program checks the layout facts the kernels rely on (ga_kernels.hpp, "Layout facts of the 256-point transforms"); a case
// outside them is reported as failed and not run.  The twiddle tables are computed as Context::init_device computes them.
// Each check prints one line, "check <name> ok|FAIL <figures> [wall time since the previous line]"; exit status 1 if any check
// fails, 3 at once after a HIP error (the caller then starts nothing more).  tests/test_gpu_rfft_ref.py holds the set of check names.
//
// The bounds (u = 2^-24 for T = float, 2^-53 for T = double; gamma_k = k u / (1 - k u); Higham, Accuracy and Stability of Numerical
// Algorithms, 2nd ed.).  Theorem 24.2: a radix-2 transform of 2^t points whose twiddles carry errors of at most mu satisfies
//   ||computed - exact||_2 <= (t eta / (1 - t eta)) ||exact||_2,   eta = mu + gamma_4 (sqrt 2 + mu);
// the tables are correctly rounded float64 values cast to T, mu = u_T.  The kernels' transform is the 256-point decimation of the real
// block into its even and odd samples, z = x_even + i x_odd: seven butterfly stages of one 128-point complex transform (the first one in
// the lane, on a zero upper half: a twiddle product and no addition), then the split X[k] = E[k] + W_256^k O[k] with E, O separated from
// Z[k] and conj Z[128 - k] -- the eighth butterfly stage of the 256-point transform, with one more addition per operand than a plain
// butterfly (the halvings are exact) where the first stage has one less.  So t = 8 = log2 256:  e_T = 8 eta_T / (1 - 8 eta_T),
// e_float = 3.17e-6, e_double = 5.9e-15.  The theorem speaks of the whole spectrum; spectrum and error are both Hermitian, and the sums
// below run over the 129 bins the kernels store.
//   forward, T = float    per (row, block):   ||got - X||_2 <= e_f ||X||_2
//   forward, T = double   per bin:            |got - X[k]| <= 2^-24 |X[k]| + 2 e_d ||X||_2      (one float rounding of a double transform)
//   inverse               per (row, block t), y_t = the exact 256 samples, h_t | g_t its halves, g_{-1} = the incoming overlap (exact floats):
//                           ||out_t - (h_t + g_{t-1})||_2 <= (e_T + 2^-24) (||y_t||_2 + ||y_{t-1}||_2) + 2^-24 ||h_t + g_{t-1}||_2
//                         (transform error, the rounding of head and tail to float, the rounding of their float sum; block 0: y_0 alone)
//                           ||overlap_out - g_{n-1}||_2 <= (e_T + 2^-24) ||y_{n-1}||_2
//                         The second chunk's reference starts from the overlap the device wrote for the first: every bound is per chunk.
//   chain                 largest error <= 2e-6 x the reference's peak (the render tests' REL, as coarse_kernels_check chain uses)
// A wrong bin, twiddle, block or row is an error of order ||X||: 1e-2 and more of these bounds' scale of 1.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "ga_kernels.hpp"
#include "rfft_ref.hpp"

using namespace ga;
namespace rr = rfft_ref;
using rr::cd;
static_assert(rr::kBins == kBins && rr::kBlock == kBlock, "tests/rfft_ref.hpp restates the block length and the bin count");

namespace ga {
[[noreturn]] void launch_fail(const char* what) {   // (ga_engine.cpp's is not linked here)
  std::printf("launch_fail: %s\n", what);
  std::exit(2);
}
}  // namespace ga

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); std::fflush(stdout); std::exit(3); } } while (0)

static int failures = 0;
static void check(const std::string& name, bool ok, const char* fmt, ...) {
  char buf[640];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  static auto last = std::chrono::steady_clock::now();   // wall time since the previous check line: device, host reference and comparison
  const auto now = std::chrono::steady_clock::now();
  std::printf("check %s %s %s [%.0f ms]\n", name.c_str(), ok ? "ok" : "FAIL", buf, std::chrono::duration<double, std::milli>(now - last).count());
  last = now;
  std::fflush(stdout);
  if (!ok) failures++;
}
static std::string fmt(const char* f, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, f);
  std::vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}

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

template <class F>
static void parallel_for(size_t n, F f) {   // the host reference: at most 16 threads
  const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::atomic<size_t> next{0};
  std::vector<std::thread> th;
  for (unsigned i = 0; i < nt; i++)
    th.emplace_back([&] {
      for (size_t k; (k = next.fetch_add(1)) < n;) f(k);
    });
  for (auto& t : th) t.join();
}

constexpr uint32_t kCD = 0xCDCDCDCDu, kNaN = 0x7FC00000u;
static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
static float from_bits(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
static bool is_cd(float f) { return bits(f) == kCD; }
static const float kNaNf = from_bits(kNaN);
static int roundup(int v, int m) { return (v + m - 1) / m * m; }

// device array between two guard regions; array and guards start as the 32-bit word `word` (0xCDCDCDCD for outputs, a NaN for inputs)
struct Guarded {
  char* raw = nullptr;
  size_t bytes, g;
  uint32_t word;
  explicit Guarded(size_t bytes_, uint32_t word_ = kCD, size_t guard = 65536) : bytes((bytes_ + 255) / 256 * 256), g(guard), word(word_) {
    CK(hipMalloc(&raw, g + bytes + g));
    reset();
  }
  void reset() { CK(hipMemsetD32((hipDeviceptr_t)raw, (int)word, (g + bytes + g) / 4)); }
  ~Guarded() { (void)hipFree(raw); }
  Guarded(const Guarded&) = delete;
  Guarded& operator=(const Guarded&) = delete;
  float* f(size_t float_off = 0) const { return (float*)(raw + g) + float_off; }
  void upload(const void* src, size_t n) { CK(hipMemcpy(raw + g, src, n, hipMemcpyHostToDevice)); }
  std::vector<float> host(size_t nfloats) const {
    std::vector<float> h(nfloats);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h.data(), raw + g, nfloats * 4, hipMemcpyDeviceToHost));
    return h;
  }
  size_t guard_damage() const {   // words of the guards that no longer hold `word`
    CK(hipDeviceSynchronize());
    size_t bad = 0;
    std::vector<uint32_t> h(g / 4);
    CK(hipMemcpy(h.data(), raw, g, hipMemcpyDeviceToHost));
    for (uint32_t v : h) bad += v != word;
    CK(hipMemcpy(h.data(), raw + g + bytes, g, hipMemcpyDeviceToHost));
    for (uint32_t v : h) bad += v != word;
    return bad;
  }
};
struct GuardedIn : Guarded {   // input between NaN guards
  explicit GuardedIn(const std::vector<float>& h) : GuardedIn(h.data(), h.size()) {}
  GuardedIn(const float* h, size_t n) : Guarded(std::max<size_t>(4, n * 4), kNaN) {
    if (n) upload(h, n * 4);
  }
};
template <class T>
struct DevIn {   // plain device table
  T* p = nullptr;
  explicit DevIn(const std::vector<T>& h) {
    CK(hipMalloc(&p, std::max<size_t>(1, h.size()) * sizeof(T)));
    if (!h.empty()) CK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  }
  ~DevIn() { (void)hipFree(p); }
  DevIn(const DevIn&) = delete;
  DevIn& operator=(const DevIn&) = delete;
};
static void sync_check() {
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
}

// twiddle tables: the formulas of Context::init_device (ga_engine.cpp)
struct TwTables {
  std::unique_ptr<DevIn<double2>> d128, d256;
  Twiddles tw;
  TwTables() {
    const double pi = 3.14159265358979323846264338327950288;
    std::vector<double2> t128(64), t256(129);
    for (int j = 0; j < 64; j++) t128[j] = make_double2(std::cos(2.0 * pi * j / 128.0), -std::sin(2.0 * pi * j / 128.0));
    for (int k = 0; k <= 128; k++) t256[k] = make_double2(std::cos(2.0 * pi * k / 256.0), -std::sin(2.0 * pi * k / 256.0));
    d128.reset(new DevIn<double2>(t128));
    d256.reset(new DevIn<double2>(t256));
    tw = Twiddles{d128->p, d256->p};
  }
};
static Twiddles gTw;

// ---- the bounds ---------------------------------------------------------------------------------------------------------------------
static const double kUf = 5.9604644775390625e-08, kUd = 1.1102230246251565e-16;
static double e_of(double u) {
  const double g4 = 4.0 * u / (1.0 - 4.0 * u), eta = u + g4 * (std::sqrt(2.0) + u);
  return 8.0 * eta / (1.0 - 8.0 * eta);
}
enum Inst { kA = 0, kB32 = 1, kB64 = 2 };
static const char* const kInstName[3] = {"a", "b32", "b64"};
static double e_inst(Inst i) { return e_of(i == kB32 ? kUf : kUd); }
static double finite_or_huge(double r) { return r == r ? r : 1e300; }

// ---- the layout facts the kernels rely on (ga_kernels.hpp); a case outside them is not launched ----------------------------------------
static const char* facts_fwd(Inst i, int nrows, int n, int hist, int tx, int rp) {
  if (nrows < 1 || n < 1 || hist < 0) return "nrows, nblocks or hist";
  if (i == kA) return rp % 128 || roundup(nrows, 32) > rp || tx < hist + n ? "A: rp is a multiple of 128 that holds the row tiles, tx >= hist + nblocks" : nullptr;
  return tx % 4 || hist % 4 || tx < hist + roundup(n, 4) ? "B: tx and hist are multiples of 4, tx >= hist + roundup(nblocks, 4)" : nullptr;
}
static const char* facts_inv(Inst i, int nrows, int n, int ty, int rp, const float* out0, size_t out_stride) {
  if (nrows < 1 || n < 1) return "nrows or nblocks";
  if (((uintptr_t)out0 | (out_stride * 4)) % 16) return "out rows are 16-byte aligned";
  if (i == kA) return rp % 128 || roundup(nrows, 32) > rp || ty < n ? "A: rp is a multiple of 128 that holds the row tiles, ty >= nblocks" : nullptr;
  return ty % 4 || ty < roundup(n, 4) ? "B: ty is a multiple of 4, ty >= roundup(nblocks, 4)" : nullptr;
}

// =====================================================================================================================
//  signals: every row is exactly n x 128 floats with at least 132 NaN behind it, in one buffer between NaN guards.  Row kinds of the
//  cases with 31 rows and more: row 3 has no buffer, 5 is all zeros, 7 is scaled by 1e-30, 9 is one impulse at sample 127 of the last
//  block, 11 is row 10's samples in a view that starts one float past a 16-byte boundary.
// =====================================================================================================================
enum { kRowNull = 3, kRowZero = 5, kRowTiny = 7, kRowImpulse = 9, kRowAligned = 10, kRowView = 11 };
struct Signals {
  int nrows, n;
  std::vector<float> buf;    // NaN where no row lies
  std::vector<long> off;     // per row: first sample in buf, -1: null
  const float* row(int r) const { return off[r] < 0 ? nullptr : buf.data() + off[r]; }
};
static Signals make_signals(int nrows, int n, uint64_t seed, bool kinds, bool equal_blocks = false) {
  Signals S;
  S.nrows = nrows;
  S.n = n;
  Rng rng{seed};
  const size_t len = (size_t)n * kBlock;
  size_t cur = 0;
  for (int r = 0; r < nrows; r++) {
    if (kinds && r == kRowNull) {
      S.off.push_back(-1);
      continue;
    }
    const size_t start = cur + (kinds && r == kRowView ? 1 : 0);
    S.buf.resize(roundup((int)(start + len + 132), 4), kNaNf);
    for (size_t i = 0; i < len; i++) {
      float v = rng.unit();
      if (equal_blocks && i >= (size_t)kBlock) v = S.buf[start + i % kBlock];
      if (kinds && r == kRowZero) v = 0.f;
      if (kinds && r == kRowTiny) v *= 1e-30f;
      if (kinds && r == kRowImpulse) v = i == len - 1 ? 1.f : 0.f;
      if (kinds && r == kRowView) v = S.buf[(size_t)S.off[kRowAligned] + i];
      S.buf[start + i] = v;
    }
    S.off.push_back((long)start);
    cur = S.buf.size();
  }
  if (S.buf.empty()) S.buf.assign(4, kNaNf);
  return S;
}
static std::vector<ConvRowIO> row_table(const Signals& S, const GuardedIn& d) {
  std::vector<ConvRowIO> io(S.nrows);
  for (int r = 0; r < S.nrows; r++) io[r] = ConvRowIO{S.off[r] < 0 ? nullptr : d.f((size_t)S.off[r]), nullptr};
  return io;
}

// ---- forward through one instance ---------------------------------------------------------------------------------------------------
struct FwdResult {
  Inst inst;
  int nrows, n, hist, tx, rp;
  std::vector<float> xr, xi;
  size_t dmg = 0;
  bool ran = false;
  size_t at(int row, int k, int t) const { return inst == kA ? rr::index_a(k, t, row, hist, tx, rp) : rr::index_b(row, k, t, hist, tx); }
};
static FwdResult run_forward(const std::string& name, Inst inst, const Signals& S, const GuardedIn& dsig, int hist, int tx) {
  FwdResult R;
  R.inst = inst; R.nrows = S.nrows; R.n = S.n; R.hist = hist; R.tx = tx; R.rp = 128;
  if (const char* why = facts_fwd(inst, S.nrows, S.n, hist, tx, R.rp)) {
    check(name, false, "not run: %s", why);
    return R;
  }
  const size_t sz = inst == kA ? (size_t)kBins * tx * R.rp : (size_t)S.nrows * kBins * tx;
  Guarded xr(sz * 4), xi(sz * 4);
  DevIn<ConvRowIO> io(row_table(S, dsig));
  if (inst == kA) launch_rfft_fwd(nullptr, io.p, S.nrows, S.n, hist, ConvPlanes{xr.f(), xi.f(), nullptr, nullptr, tx, 0, R.rp}, gTw);
  else launch_rfft_fwd_b(nullptr, io.p, S.nrows, S.n, hist, ConvPlanesB{xr.f(), xi.f(), nullptr, nullptr, tx, 0}, gTw, inst == kB64);
  sync_check();
  R.xr = xr.host(sz);
  R.xi = xi.host(sz);
  R.dmg = xr.guard_damage() + xi.guard_damage();
  R.ran = true;
  return R;
}
// float64 spectra of every (row, block): [row][block][129]
static std::vector<cd> forward_reference(const Signals& S) {
  std::vector<cd> X((size_t)S.nrows * S.n * kBins);
  parallel_for((size_t)S.nrows * S.n, [&](size_t i) {
    const float* row = S.row((int)(i / S.n));
    rr::forward(row ? row + (i % S.n) * kBlock : nullptr, X.data() + i * kBins);
  });
  return X;
}
struct FwdTally {
  double ratio = 0.0;
  long not_nearest = 0, elements = 0, im_edge = 0, silent_nonzero = 0, nan = 0, pad_nonzero = 0, pad_nan = 0, stray = 0;
  bool clean() const { return ratio <= 1.0 && !im_edge && !silent_nonzero && !nan && !pad_nonzero && !stray; }
};
// values against the reference, then every other element of the planes
static FwdTally judge_forward(const FwdResult& R, const std::vector<cd>& X, const Signals& S) {
  FwdTally T;
  const double eT = e_inst(R.inst);
  for (int row = 0; row < R.nrows; row++)
    for (int t = 0; t < R.n; t++) {
      const cd* x = X.data() + ((size_t)row * R.n + t) * kBins;
      double n2 = 0.0, e2 = 0.0, worst = 0.0;
      for (int k = 0; k < kBins; k++) n2 += x[k].re * x[k].re + x[k].im * x[k].im;
      const double norm = std::sqrt(n2);
      for (int k = 0; k < kBins; k++) {
        const float gr = R.xr[R.at(row, k, t)], gi = R.xi[R.at(row, k, t)];
        T.nan += (gr != gr) + (gi != gi);
        if ((k == 0 || k == kBlock) && gi != 0.f) T.im_edge++;
        if (norm == 0.0) {   // null and zero rows: zero in value
          T.silent_nonzero += (gr != 0.f) + (gi != 0.f);
          continue;
        }
        const double dr = (double)gr - x[k].re, di = (double)gi - x[k].im;
        e2 += dr * dr + di * di;
        T.not_nearest += (gr != (float)x[k].re) + (gi != (float)x[k].im);
        T.elements += 2;
        if (R.inst != kB32) worst = std::max(worst, finite_or_huge(std::hypot(dr, di) / (kUf * std::hypot(x[k].re, x[k].im) + 2.0 * eT * norm)));
      }
      if (norm != 0.0 && R.inst == kB32) worst = finite_or_huge(std::sqrt(e2) / (eT * norm));
      T.ratio = std::max(T.ratio, worst);
    }
  // what else the planes hold
  if (R.inst == kA) {
    const int rows_written = roundup(R.nrows, 32);   // the row tile's padding rows are transformed as silence
    for (int k = 0; k < kBins; k++)
      for (int c = 0; c < R.tx; c++)
        for (int r = 0; r < R.rp; r++) {
          const size_t o = ((size_t)k * R.tx + c) * R.rp + r;
          const bool col = c >= R.hist && c < R.hist + R.n;
          if (col && r < R.nrows) continue;
          if (col && r < rows_written) {
            T.pad_nonzero += !(R.xr[o] == 0.f) + !(R.xi[o] == 0.f);   // (a NaN counts, and is counted again by itself)
            T.pad_nan += (R.xr[o] != R.xr[o]) + (R.xi[o] != R.xi[o]);
          }
          else T.stray += !is_cd(R.xr[o]) + !is_cd(R.xi[o]);
        }
  } else {
    for (int row = 0; row < R.nrows; row++)
      for (int k = 0; k < kBins; k++)
        for (int c = 0; c < R.tx; c++) {
          const size_t o = ((size_t)row * kBins + k) * R.tx + c;
          if (c >= R.hist && c < R.hist + R.n) continue;
          if (c >= R.hist + R.n && c < R.hist + roundup(R.n, 4)) {
            T.pad_nonzero += !(R.xr[o] == 0.f) + !(R.xi[o] == 0.f);
            T.pad_nan += (R.xr[o] != R.xr[o]) + (R.xi[o] != R.xi[o]);
          }
          else T.stray += !is_cd(R.xr[o]) + !is_cd(R.xi[o]);
        }
  }
  (void)S;
  return T;
}
static long rows_differ(const FwdResult& R, int ra, int rb) {
  long bad = 0;
  for (int k = 0; k < kBins; k++)
    for (int t = 0; t < R.n; t++) bad += (bits(R.xr[R.at(ra, k, t)]) != bits(R.xr[R.at(rb, k, t)])) + (bits(R.xi[R.at(ra, k, t)]) != bits(R.xi[R.at(rb, k, t)]));
  return bad;
}

static void run_fwd_case(int nrows, int n, int histB, int histA) {
  const bool kinds = nrows >= 31;
  const Signals S = make_signals(nrows, n, 0xF0000u + (uint64_t)nrows * 1009 + n * 17 + histB, kinds);
  GuardedIn dsig(S.buf);
  const std::vector<cd> X = forward_reference(S);
  for (Inst inst : {kA, kB32, kB64}) {
    const int hist = inst == kA ? histA : histB;
    const int tx = inst == kA ? hist + n + 2 : hist + roundup(n, 4) + 4;
    const std::string name = fmt("fwd.r%d.n%d.h%d.%s", nrows, n, hist, kInstName[inst]);
    const FwdResult R = run_forward(name, inst, S, dsig, hist, tx);
    if (!R.ran) continue;
    const FwdTally T = judge_forward(R, X, S);
    const long view = kinds ? rows_differ(R, kRowAligned, kRowView) : 0;
    check(name, T.clean() && !view && !R.dmg,
          "ratio %.4f of the bound (e %.3e), not nearest float %ld of %ld, nan %ld im(0|128) %ld silent rows nonzero %ld padding nonzero %ld (nan %ld) stray %ld unaligned view differs %ld guard %zu",
          T.ratio, e_inst(inst), T.not_nearest, T.elements, T.nan, T.im_edge, T.silent_nonzero, T.pad_nonzero, T.pad_nan, T.stray, view, R.dmg);
  }
}
// every row count x every block count x every hist pair: 135 cases, each through the three instances.  Rows 31, 32, 33 and 65 end
// inside, at and behind a row tile of A; blocks 3, 4, 5 a quad of B, 31, 32, 33 and 64, 65 a run of 32.
static void family_fwd() {
  const int histB[3] = {0, 4, 512}, histA[3] = {0, 1, 7};
  for (int nrows : {1, 31, 32, 33, 65})
    for (int n : {1, 3, 4, 5, 31, 32, 33, 64, 65})
      for (int h = 0; h < 3; h++) run_fwd_case(nrows, n, histB[h], histA[h]);
}

// =====================================================================================================================
//  inverse.  Spectra are given as [row][bin][ntot] host arrays; a launch takes columns [t0, t0 + n) of them into planes of its own
//  (B: [row][bin][ty] with NaN from block n on; A: [bin][ty][128] with NaN from block n on and from row nrows on).
// =====================================================================================================================
struct Spectra {
  int nrows, ntot;
  std::vector<float> re, im;   // [row][bin][ntot]
  size_t at(int row, int k, int t) const { return ((size_t)row * kBins + k) * ntot + t; }
};
enum { kOutNull = 3, kSpecZero = 5, kSpecTiny = 7 };   // row kinds of the cases with 33 rows and more
static Spectra make_spectra(int nrows, int ntot, Rng& rng, bool kinds, bool equal_columns = false) {
  Spectra Y;
  Y.nrows = nrows;
  Y.ntot = ntot;
  Y.re.resize((size_t)nrows * kBins * ntot);
  Y.im.resize(Y.re.size());
  for (int r = 0; r < nrows; r++) {
    const float sc = kinds && r == kSpecZero ? 0.f : (kinds && r == kSpecTiny ? 1e-30f : 1.f);
    for (int k = 0; k < kBins; k++)
      for (int t = 0; t < ntot; t++) {
        const size_t o = Y.at(r, k, t);
        if (equal_columns && t > 0) {
          Y.re[o] = Y.re[o - t];
          Y.im[o] = Y.im[o - t];
        } else {
          Y.re[o] = rng.unit() * sc;   // (Im of bins 0 and 128 is non-zero: the contract ignores it)
          Y.im[o] = rng.unit() * sc;
        }
      }
  }
  return Y;
}
struct InvResult {
  std::vector<float> out;   // [nrows][n x 128]; a row without an output keeps 0xCD
  std::vector<float> ov;    // [nrows][128]
  size_t dmg = 0;
  bool ran = false;
};
static InvResult run_inverse(const std::string& name, Inst inst, const Spectra& Y, int t0, int n, const std::vector<float>& ov_in, bool null_row, int ty_force = 0) {
  InvResult R;
  const int nrows = Y.nrows, rp = 128;
  const int ty = ty_force ? ty_force : (inst == kA ? n + 3 : roundup(n, 4) + 4);
  const size_t olen = (size_t)n * kBlock;
  Guarded out((size_t)nrows * olen * 4), ovo((size_t)nrows * kBlock * 4);
  if (const char* why = facts_inv(inst, nrows, n, ty, rp, out.f(), olen)) {
    check(name, false, "not run: %s", why);
    return R;
  }
  const size_t psz = inst == kA ? (size_t)kBins * ty * rp : (size_t)nrows * kBins * ty;
  std::vector<float> pr(psz, kNaNf), pi(psz, kNaNf);
  for (int r = 0; r < nrows; r++)
    for (int k = 0; k < kBins; k++)
      for (int t = 0; t < n; t++) {
        const size_t o = inst == kA ? rr::index_a(k, t, r, 0, ty, rp) : rr::index_b(r, k, t, 0, ty);
        pr[o] = Y.re[Y.at(r, k, t0 + t)];
        pi[o] = Y.im[Y.at(r, k, t0 + t)];
      }
  GuardedIn dpr(pr), dpi(pi), dov(ov_in);
  std::vector<ConvRowIO> io(nrows);
  std::vector<const float*> oin(nrows);
  std::vector<float*> oout(nrows);
  for (int r = 0; r < nrows; r++) {
    io[r] = ConvRowIO{nullptr, null_row && r == kOutNull ? nullptr : out.f(r * olen)};
    oin[r] = dov.f((size_t)r * kBlock);
    oout[r] = ovo.f((size_t)r * kBlock);
  }
  DevIn<ConvRowIO> dio(io);
  DevIn<const float*> doin(oin);
  DevIn<float*> doout(oout);
  if (inst == kA) launch_irfft_ola(nullptr, dio.p, nrows, n, ConvPlanes{nullptr, nullptr, dpr.f(), dpi.f(), 0, ty, rp}, dov.f(), ovo.f(), gTw);
  else launch_irfft_ola_b(nullptr, dio.p, nrows, n, ConvPlanesB{nullptr, nullptr, dpr.f(), dpi.f(), 0, ty}, doin.p, doout.p, gTw, inst == kB64);
  sync_check();
  R.out = out.host((size_t)nrows * olen);
  R.ov = ovo.host((size_t)nrows * kBlock);
  R.dmg = out.guard_damage() + ovo.guard_damage();
  R.ran = true;
  return R;
}
// the exact 256 samples of columns [t0, t0 + n) of every row: [row][n][256]
static std::vector<double> inverse_reference(const Spectra& Y, int t0, int n) {
  std::vector<double> y((size_t)Y.nrows * n * rr::kN);
  parallel_for((size_t)Y.nrows * n, [&](size_t i) {
    const int r = (int)(i / n), t = (int)(i % n);
    cd s[kBins];
    for (int k = 0; k < kBins; k++) s[k] = cd{Y.re[Y.at(r, k, t0 + t)], Y.im[Y.at(r, k, t0 + t)]};
    rr::inverse(s, y.data() + i * rr::kN);
  });
  return y;
}
struct InvTally {
  double ratio = 0.0, ov_ratio = 0.0;
  long nan = 0, unwritten = 0, null_written = 0;
  bool clean() const { return ratio <= 1.0 && ov_ratio <= 1.0 && !nan && !unwritten && !null_written; }
  void merge(const InvTally& o) {
    ratio = std::max(ratio, o.ratio); ov_ratio = std::max(ov_ratio, o.ov_ratio);
    nan += o.nan; unwritten += o.unwritten; null_written += o.null_written;
  }
};
static double norm2(const double* v, int n) {
  double s = 0.0;
  for (int i = 0; i < n; i++) s += v[i] * v[i];
  return std::sqrt(s);
}
static InvTally judge_inverse(Inst inst, const InvResult& R, const std::vector<double>& y, int nrows, int n, const std::vector<float>& ov_in, bool null_row) {
  InvTally T;
  const double c = e_inst(inst) + kUf;
  for (int r = 0; r < nrows; r++) {
    const double* yr = y.data() + (size_t)r * n * rr::kN;
    const float* out = R.out.data() + (size_t)r * n * kBlock;
    if (null_row && r == kOutNull) {
      for (size_t i = 0; i < (size_t)n * kBlock; i++) T.null_written += !is_cd(out[i]);
    } else {
      for (int t = 0; t < n; t++) {
        double want[kBlock], diff[kBlock];
        for (int i = 0; i < kBlock; i++) {
          const float g = out[(size_t)t * kBlock + i];
          T.nan += g != g;
          T.unwritten += is_cd(g);
          want[i] = yr[(size_t)t * rr::kN + i] + (t ? yr[(size_t)(t - 1) * rr::kN + kBlock + i] : (double)ov_in[(size_t)r * kBlock + i]);
          diff[i] = (double)g - want[i];
        }
        const double bound = c * (norm2(yr + (size_t)t * rr::kN, rr::kN) + (t ? norm2(yr + (size_t)(t - 1) * rr::kN, rr::kN) : 0.0)) + kUf * norm2(want, kBlock);
        const double err = norm2(diff, kBlock);
        T.ratio = std::max(T.ratio, bound > 0.0 ? finite_or_huge(err / bound) : (err == 0.0 ? 0.0 : 1e300));
      }
    }
    double diff[kBlock];
    for (int i = 0; i < kBlock; i++) {
      const float g = R.ov[(size_t)r * kBlock + i];
      T.nan += g != g;
      T.unwritten += is_cd(g);
      diff[i] = (double)g - yr[(size_t)(n - 1) * rr::kN + kBlock + i];
    }
    const double bound = c * norm2(yr + (size_t)(n - 1) * rr::kN, rr::kN), err = norm2(diff, kBlock);
    T.ov_ratio = std::max(T.ov_ratio, bound > 0.0 ? finite_or_huge(err / bound) : (err == 0.0 ? 0.0 : 1e300));
  }
  return T;
}
static std::vector<float> random_overlap(int nrows, Rng& rng, bool kinds) {
  std::vector<float> ov((size_t)nrows * kBlock);
  for (int r = 0; r < nrows; r++)
    for (int i = 0; i < kBlock; i++) ov[(size_t)r * kBlock + i] = rng.unit() * (kinds && r == kSpecTiny ? 1e-30f : 1.f);
  return ov;
}
// two chunks of n blocks: the first from a random overlap, the second from the overlap the device wrote
static void run_inv_case(const std::string& tag, int nrows, int n, int ty_force = 0) {
  const bool kinds = nrows >= 33;
  Rng rng{0x1F0000u + (uint64_t)nrows * 1009 + n * 17};
  const Spectra Y = make_spectra(nrows, 2 * n, rng, kinds);
  const std::vector<float> ov0 = random_overlap(nrows, rng, kinds);
  const std::vector<double> y0 = inverse_reference(Y, 0, n), y1 = inverse_reference(Y, n, n);
  for (Inst inst : {kA, kB32, kB64}) {
    if (ty_force && inst == kA) continue;   // (the migration launch is formulation B's)
    const std::string name = tag + "." + kInstName[inst];
    const InvResult R0 = run_inverse(name, inst, Y, 0, n, ov0, kinds, ty_force);
    if (!R0.ran) continue;
    const InvResult R1 = run_inverse(name, inst, Y, n, n, R0.ov, kinds, ty_force);
    if (!R1.ran) continue;
    InvTally T = judge_inverse(inst, R0, y0, nrows, n, ov0, kinds);
    const InvTally T1 = judge_inverse(inst, R1, y1, nrows, n, R0.ov, kinds);
    const double r0 = T.ratio, r1 = T1.ratio;
    T.merge(T1);
    check(name, T.clean() && !R0.dmg && !R1.dmg,
          "ratio %.4f of the bound (chunk 1 %.4f, chunk 2 %.4f; e + 2^-24 = %.3e), overlap ratio %.4f, nan %ld unwritten %ld written without an output %ld guard %zu",
          T.ratio, r0, r1, e_inst(inst) + kUf, T.ov_ratio, T.nan, T.unwritten, T.null_written, R0.dmg + R1.dmg);
  }
}
// every row count x every block count.  160 blocks are five full runs: the 33rd transform lands on waves 0, 1, 2, 3, 0.
static void family_inv() {
  for (int nrows : {1, 33, 65})
    for (int n : {1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 160, 161}) run_inv_case(fmt("inv.r%d.n%d", nrows, n), nrows, n);
  run_inv_case("inv.migrate", 3, 1, kRebuildTy);   // planConvMigration's launch: one block on planes of kRebuildTy = 4 columns
}

// =====================================================================================================================
//  exact
// =====================================================================================================================
static void family_exact() {
  // (i) equal blocks -> equal columns
  {
    const int n = 161, nrows = 2;
    const Signals S = make_signals(nrows, n, 0xE0001u, false, true);
    GuardedIn dsig(S.buf);
    for (Inst inst : {kA, kB32, kB64}) {
      const int hist = inst == kA ? 1 : 4, tx = inst == kA ? hist + n + 2 : hist + roundup(n, 4) + 4;
      const std::string name = fmt("exact.fwd_columns.%s", kInstName[inst]);
      const FwdResult R = run_forward(name, inst, S, dsig, hist, tx);
      if (!R.ran) continue;
      long bad = 0, first = -1;
      for (int r = 0; r < nrows; r++)
        for (int k = 0; k < kBins; k++)
          for (int t = 1; t < n; t++) {
            const bool d = bits(R.xr[R.at(r, k, t)]) != bits(R.xr[R.at(r, k, 0)]) || bits(R.xi[R.at(r, k, t)]) != bits(R.xi[R.at(r, k, 0)]);
            if (d && first < 0) first = t;
            bad += d;
          }
      check(name, !bad && !R.dmg, "columns that differ from column 0: %ld (first at block %ld) guard %zu", bad, first, R.dmg);
    }
  }
  // (ii) equal columns, the incoming overlap the tail those columns give -> equal blocks, and the same tail again
  {
    const int n = 161, nrows = 2;
    Rng rng{0xE0002u};
    const Spectra Y = make_spectra(nrows, n, rng, false, true);
    const std::vector<float> any = random_overlap(nrows, rng, false);
    for (Inst inst : {kA, kB32, kB64}) {
      const std::string name = fmt("exact.inv_columns.%s", kInstName[inst]);
      const InvResult one = run_inverse(name, inst, Y, 0, 1, any, false);   // its outgoing overlap: the tail of column 0
      if (!one.ran) continue;
      const InvResult R = run_inverse(name, inst, Y, 0, n, one.ov, false);
      if (!R.ran) continue;
      long bad = 0, first = -1, ovbad = 0;
      for (int r = 0; r < nrows; r++) {
        const float* out = R.out.data() + (size_t)r * n * kBlock;
        for (int t = 1; t < n; t++) {
          bool d = false;
          for (int i = 0; i < kBlock; i++) d = d || bits(out[(size_t)t * kBlock + i]) != bits(out[i]);
          if (d && first < 0) first = t;
          bad += d;
        }
        for (int i = 0; i < kBlock; i++) ovbad += bits(R.ov[(size_t)r * kBlock + i]) != bits(one.ov[(size_t)r * kBlock + i]);
      }
      check(name, !bad && !ovbad && !R.dmg && !one.dmg, "blocks that differ from block 0: %ld (first %ld), overlap samples that differ %ld, guard %zu", bad, first, ovbad,
            R.dmg + one.dmg);
    }
  }
  // (iii) one chunk of n blocks against the same blocks in two chunks chained through the overlap
  for (int n : {97, 161}) {
    const int nrows = 2;
    Rng rng{0xE0003u + (uint64_t)n};
    const Spectra Y = make_spectra(nrows, n, rng, false);
    const std::vector<float> ov0 = random_overlap(nrows, rng, false);
    for (Inst inst : {kA, kB32, kB64}) {
      const std::string name = fmt("exact.split.n%d.%s", n, kInstName[inst]);
      const InvResult whole = run_inverse(name, inst, Y, 0, n, ov0, false);
      if (!whole.ran) continue;
      long bad[3] = {0, 0, 0};
      size_t dmg = whole.dmg;
      bool ran = true;
      int si = 0;
      for (int s : {1, 32, 33}) {
        const InvResult a = run_inverse(name, inst, Y, 0, s, ov0, false);
        if (!a.ran) { ran = false; break; }
        const InvResult b = run_inverse(name, inst, Y, s, n - s, a.ov, false);
        if (!b.ran) { ran = false; break; }
        dmg += a.dmg + b.dmg;
        for (int r = 0; r < nrows; r++) {
          for (size_t i = 0; i < (size_t)n * kBlock; i++) {
            const float g = i < (size_t)s * kBlock ? a.out[(size_t)r * s * kBlock + i] : b.out[(size_t)r * (n - s) * kBlock + i - (size_t)s * kBlock];
            bad[si] += bits(g) != bits(whole.out[(size_t)r * n * kBlock + i]);
          }
          for (int i = 0; i < kBlock; i++) bad[si] += bits(b.ov[(size_t)r * kBlock + i]) != bits(whole.ov[(size_t)r * kBlock + i]);
        }
        si++;
      }
      if (!ran) continue;
      check(name, !bad[0] && !bad[1] && !bad[2] && !dmg, "samples that differ from the one-chunk run: split at 1: %ld, at 32: %ld, at 33: %ld, guard %zu", bad[0], bad[1],
            bad[2], dmg);
    }
  }
}

// =====================================================================================================================
//  seam: 65,537 rows / jobs, n = 1, hist = 0, tx = ty = 4.  The launchers cut their grid at 65,535 rows: rows 65,535 and 65,536 come
//  from the second launch.  Row 0 is held to the reference, every other row to row 0's bits.
// =====================================================================================================================
static std::string seam_rows(const std::vector<float>& a, const std::vector<float>& b, size_t stride, int nrows, long& bad) {
  bad = 0;
  std::string named;
  for (int r = 1; r < nrows; r++) {
    const bool d = std::memcmp(a.data() + (size_t)r * stride, a.data(), stride * 4) || std::memcmp(b.data() + (size_t)r * stride, b.data(), stride * 4);
    bad += d;
    if (r >= nrows - 3) named += fmt(" row %d %s", r, d ? "differs" : "equal");
  }
  return named;
}
static void family_seam() {
  const int N = 65537, tx = 4, ty = 4;
  const auto t0 = std::chrono::steady_clock::now();
  const Signals S = make_signals(1, 1, 0x5EA0001u, false);
  GuardedIn dsig(S.buf);
  const std::vector<cd> X = forward_reference(S);
  {
    const size_t sz = (size_t)N * kBins * tx;
    Guarded xr(sz * 4), xi(sz * 4);
    DevIn<ConvRowIO> io(std::vector<ConvRowIO>((size_t)N, ConvRowIO{dsig.f((size_t)S.off[0]), nullptr}));
    std::vector<ConvRebuildJob> jobs((size_t)N);
    Guarded store(256);   // P = 1: the [129][P - 1] store is empty
    for (int j = 0; j < N; j++) jobs[j] = ConvRebuildJob{dsig.f((size_t)S.off[0]), store.f(), store.f(), 1, j};
    DevIn<ConvRebuildJob> djobs(jobs);
    for (int pass = 0; pass < 3; pass++) {   // B<float>, B<double>, the rebuild
      const std::string name = pass == 0 ? "seam.fwd_b32" : (pass == 1 ? "seam.fwd_b64" : "seam.rebuild");
      const Inst inst = pass == 0 ? kB32 : kB64;
      if (const char* why = facts_fwd(inst, N, 1, 0, tx, 128)) { check(name, false, "not run: %s", why); continue; }
      xr.reset();
      xi.reset();
      if (pass < 2) launch_rfft_fwd_b(nullptr, io.p, N, 1, 0, ConvPlanesB{xr.f(), xi.f(), nullptr, nullptr, tx, ty}, gTw, pass == 1);
      else launch_conv_rebuild(nullptr, djobs.p, N, 1, ConvPlanesB{xr.f(), xi.f(), nullptr, nullptr, conv_rebuild_tx(1), kRebuildTy}, conv_rebuild_hist(1), gTw);
      sync_check();
      FwdResult R;
      R.inst = inst; R.nrows = 1; R.n = 1; R.hist = 0; R.tx = tx; R.rp = 128;
      R.xr = xr.host(sz);
      R.xi = xi.host(sz);
      FwdTally T = judge_forward(R, X, S);   // row 0 (the walk stays inside row 0's 129 x 4 elements)
      if (pass == 2) {   // the rebuild writes the job's own block and nothing else: columns 1 to 3 still read 0xCD
        T.pad_nonzero = 0;
        for (int k = 0; k < kBins; k++)
          for (int c = 1; c < tx; c++) T.stray += !is_cd(R.xr[(size_t)k * tx + c]) + !is_cd(R.xi[(size_t)k * tx + c]);
      }
      long bad;
      const std::string named = seam_rows(R.xr, R.xi, (size_t)kBins * tx, N, bad);
      const size_t dmg = xr.guard_damage() + xi.guard_damage() + store.guard_damage();
      check(name, T.clean() && !bad && !dmg, "row 0: ratio %.4f of the bound, nan %ld padding nonzero %ld (nan %ld) stray %ld; rows that differ from row 0: %ld of %d;%s; guard %zu", T.ratio,
            T.nan, T.pad_nonzero, T.pad_nan, T.stray, bad, N - 1, named.c_str(), dmg);
    }
  }
  {
    Rng rng{0x5EA0002u};
    const Spectra Y1 = make_spectra(1, 1, rng, false);
    const std::vector<float> ov1 = random_overlap(1, rng, false);
    const std::vector<double> y = inverse_reference(Y1, 0, 1);
    const size_t rowsz = (size_t)kBins * ty, sz = (size_t)N * rowsz;
    std::vector<float> pr(sz, kNaNf), pi(sz, kNaNf), ov((size_t)N * kBlock);
    for (int r = 0; r < N; r++) {
      for (int k = 0; k < kBins; k++) {
        pr[(size_t)r * rowsz + (size_t)k * ty] = Y1.re[k];
        pi[(size_t)r * rowsz + (size_t)k * ty] = Y1.im[k];
      }
      std::memcpy(ov.data() + (size_t)r * kBlock, ov1.data(), kBlock * 4);
    }
    GuardedIn dpr(pr), dpi(pi), dov(ov);
    std::vector<float>().swap(pr);
    std::vector<float>().swap(pi);
    Guarded out((size_t)N * kBlock * 4), ovo((size_t)N * kBlock * 4);
    std::vector<ConvRowIO> io((size_t)N);
    std::vector<const float*> oin((size_t)N);
    std::vector<float*> oout((size_t)N);
    for (int r = 0; r < N; r++) {
      io[r] = ConvRowIO{nullptr, out.f((size_t)r * kBlock)};
      oin[r] = dov.f((size_t)r * kBlock);
      oout[r] = ovo.f((size_t)r * kBlock);
    }
    DevIn<ConvRowIO> dio(io);
    DevIn<const float*> doin(oin);
    DevIn<float*> doout(oout);
    for (Inst inst : {kB32, kB64}) {
      const std::string name = fmt("seam.inv_%s", kInstName[inst]);
      if (const char* why = facts_inv(inst, N, 1, ty, 128, out.f(), kBlock)) { check(name, false, "not run: %s", why); continue; }
      out.reset();
      ovo.reset();
      launch_irfft_ola_b(nullptr, dio.p, N, 1, ConvPlanesB{nullptr, nullptr, dpr.f(), dpi.f(), tx, ty}, doin.p, doout.p, gTw, inst == kB64);
      sync_check();
      InvResult R;
      R.out = out.host((size_t)N * kBlock);
      R.ov = ovo.host((size_t)N * kBlock);
      const InvTally T = judge_inverse(inst, R, y, 1, 1, ov1, false);   // row 0
      long bad;
      const std::string named = seam_rows(R.out, R.ov, kBlock, N, bad);
      const size_t dmg = out.guard_damage() + ovo.guard_damage();
      check(name, T.clean() && !bad && !dmg, "row 0: ratio %.4f of the bound, overlap ratio %.4f, nan %ld unwritten %ld; rows that differ from row 0: %ld of %d;%s; guard %zu",
            T.ratio, T.ov_ratio, T.nan, T.unwritten, bad, N - 1, named.c_str(), dmg);
    }
  }
  std::printf("seam took %.2f s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
}

// =====================================================================================================================
//  chain: P = 5 partitions (640 taps), two chunks of 33 and 40 blocks, uniform input and taps.
//  B: planes as PrivateStage lays them out (tx = hist + roundup(n, 16) + 16, ty = roundup(n, 256), hist = roundup(P - 1, 4)); the
//     history columns and the columns behind the chunk are set by launch_hist_copy_b as the stage's restore jobs do, the second chunk's
//     history read from the first chunk's planes where it lies.  The taps' spectra are launch_rfft_fwd_b's (fp64), repacked [bin][P].
//  A: three rows on one impulse response; planes as planConvolversShared makes them (ty = roundup(n, 64), tx = ty + P + 128, hist = P - 1,
//     the history and the zeroed rows behind the chunk by launch_plane_copy); the taps through launch_rfft_fwd and launch_extract_ir.
// =====================================================================================================================
constexpr int kChainP = 5, kChainN[2] = {33, 40}, kChainBlocks = 73;
static std::vector<double> direct_convolution(const float* x, size_t nx, const std::vector<float>& h) {
  std::vector<double> want(nx);
  parallel_for((nx + 255) / 256, [&](size_t blk) {
    for (size_t i = blk * 256; i < std::min(nx, (blk + 1) * 256); i++) {
      double acc = 0.0;
      for (size_t j = 0; j < h.size() && j <= i; j++) acc += (double)h[j] * (double)x[i - j];
      want[i] = acc;
    }
  });
  return want;
}
static void chain_report(const std::string& name, const std::vector<float>& got, const std::vector<double>& want, size_t dmg) {
  double peak = 0.0, worst = 0.0, e2 = 0.0, n2 = 0.0;
  size_t unwritten = 0, nan = 0;
  for (size_t i = 0; i < want.size(); i++) {
    unwritten += is_cd(got[i]);
    nan += got[i] != got[i];
    peak = std::max(peak, std::fabs(want[i]));
    worst = std::max(worst, std::fabs(got[i] - want[i]));
    e2 += (got[i] - want[i]) * (got[i] - want[i]);
    n2 += want[i] * want[i];
  }
  check(name, !unwritten && !nan && !dmg && worst <= 2e-6 * peak, "max_err/peak %.3e bound 2e-6 ratio %.4f rms_err/rms %.3e unwritten %zu nan %zu guard %zu", worst / peak,
        worst / peak / 2e-6, std::sqrt(e2 / n2), unwritten, nan, dmg);
}
static void chain_b(bool fp64, const Signals& X, const GuardedIn& dx, const Signals& H, const GuardedIn& dh, const std::vector<double>& want) {
  const std::string name = fp64 ? "chain.b64" : "chain.b32";
  const int P = kChainP, hist = roundup(P - 1, 4), h = P - 1;
  // the taps' spectra [bin][P]
  const int txh = roundup(P, 4) + 4;
  const FwdResult T = run_forward(name, kB64, H, dh, 0, txh);
  if (!T.ran) return;
  std::vector<float> hr((size_t)kBins * P), hi(hr.size());
  for (int k = 0; k < kBins; k++)
    for (int p = 0; p < P; p++) {
      hr[(size_t)k * P + p] = T.xr[T.at(0, k, p)];
      hi[(size_t)k * P + p] = T.xi[T.at(0, k, p)];
    }
  GuardedIn dhr(hr), dhi(hi);
  Guarded out((size_t)kChainBlocks * kBlock * 4);
  GuardedIn ov0(std::vector<float>(kBlock, 0.f));
  Guarded ov1(kBlock * 4), ov2(kBlock * 4);
  float* ovs[3] = {ov0.f(), ov1.f(), ov2.f()};
  std::vector<std::unique_ptr<Guarded>> keep;
  size_t dmg = 0;
  int done = 0, prev_tx = 0, prev_n = 0;
  float *prev_xr = nullptr, *prev_xi = nullptr;
  for (int c = 0; c < 2; c++) {
    const int n = kChainN[c], tx = hist + roundup(n, 16) + 16, ty = roundup(n, 256);
    const char* why = facts_fwd(fp64 ? kB64 : kB32, 1, n, hist, tx, 128);
    if (!why) why = facts_inv(fp64 ? kB64 : kB32, 1, n, ty, 128, out.f((size_t)done * kBlock), 0);
    if (why) { check(name, false, "not run: %s", why); return; }
    Guarded* xr = new Guarded((size_t)kBins * tx * 4);
    keep.emplace_back(xr);
    Guarded* xi = new Guarded((size_t)kBins * tx * 4);
    keep.emplace_back(xi);
    Guarded* yr = new Guarded((size_t)kBins * ty * 4);
    keep.emplace_back(yr);
    Guarded* yi = new Guarded((size_t)kBins * ty * 4);
    keep.emplace_back(yi);
    const int tailn = tx - (hist + n);
    std::vector<HistJobB> jobs = {
        HistJobB{xr->f(hist - h), c ? prev_xr + hist + prev_n - h : nullptr, tx, prev_tx, h, 0},
        HistJobB{xi->f(hist - h), c ? prev_xi + hist + prev_n - h : nullptr, tx, prev_tx, h, 0},
        HistJobB{xr->f(hist + n), nullptr, tx, 0, tailn, 0},
        HistJobB{xi->f(hist + n), nullptr, tx, 0, tailn, 0},
    };
    DevIn<HistJobB> dj(jobs);
    const ConvPlanesB pl{xr->f(), xi->f(), yr->f(), yi->f(), tx, ty};
    DevIn<ConvRowIO> xio(std::vector<ConvRowIO>{ConvRowIO{dx.f((size_t)X.off[0] + (size_t)done * kBlock), nullptr}});
    DevIn<ConvRowIO> yio(std::vector<ConvRowIO>{ConvRowIO{nullptr, out.f((size_t)done * kBlock)}});
    ConvSetB S{};
    S.x = 0; S.y0 = 0; S.ncol = 1; S.P = P;
    S.hr[0] = dhr.f();
    S.hi[0] = dhi.f();
    DevIn<ConvSetB> ds(std::vector<ConvSetB>{S});
    DevIn<const float*> oin(std::vector<const float*>{ovs[c]});
    DevIn<float*> oout(std::vector<float*>{ovs[c + 1]});
    launch_hist_copy_b(nullptr, dj.p, 4, std::max(std::max(hist, tailn), 1));
    launch_rfft_fwd_b(nullptr, xio.p, 1, n, hist, pl, gTw, fp64);
    launch_spectral_mac_b(nullptr, ds.p, 1, n, hist, pl);
    launch_irfft_ola_b(nullptr, yio.p, 1, n, pl, oin.p, oout.p, gTw, fp64);
    sync_check();
    prev_xr = xr->f(); prev_xi = xi->f(); prev_tx = tx; prev_n = n;
    done += n;
  }
  for (auto& g : keep) dmg += g->guard_damage();
  dmg += out.guard_damage() + ov1.guard_damage() + ov2.guard_damage();
  chain_report(name, out.host((size_t)kChainBlocks * kBlock), want, dmg);
}
static void chain_a(const Signals& X, const GuardedIn& dx, const Signals& H, const GuardedIn& dh, const std::vector<double>& want) {
  const std::string name = "chain.a";
  const int P = kChainP, hist = P - 1, rp = 128, nrows = X.nrows;
  const size_t rowlen = (size_t)kChainBlocks * kBlock;
  // the taps: forward with hist = 0 into planes of P blocks, then h[c][k][p] = x[k][p][c]
  const FwdResult T = run_forward(name, kA, H, dh, 0, P);
  if (!T.ran) return;
  GuardedIn txr(T.xr), txi(T.xi);
  Guarded hr((size_t)kBins * P * 4), hi((size_t)kBins * P * 4);
  launch_extract_ir(nullptr, hr.f(), hi.f(), txr.f(), txi.f(), P, rp, P, 1);
  sync_check();
  Guarded out((size_t)nrows * rowlen * 4), hR((size_t)kBins * hist * rp * 4), hI((size_t)kBins * hist * rp * 4);
  GuardedIn ov0(std::vector<float>((size_t)nrows * kBlock, 0.f));
  Guarded ov1((size_t)nrows * kBlock * 4), ov2((size_t)nrows * kBlock * 4);
  float* ovs[3] = {ov0.f(), ov1.f(), ov2.f()};
  size_t dmg = 0;
  int done = 0;
  for (int c = 0; c < 2; c++) {
    const int n = kChainN[c], ty = roundup(n, 64), tx = ty + P + 128;
    const char* why = facts_fwd(kA, nrows, n, hist, tx, rp);
    if (!why) why = facts_inv(kA, nrows, n, ty, rp, out.f((size_t)done * kBlock), rowlen);
    if (why) { check(name, false, "not run: %s", why); return; }
    Guarded xr((size_t)kBins * tx * rp * 4), xi((size_t)kBins * tx * rp * 4), yr((size_t)kBins * ty * rp * 4), yi((size_t)kBins * ty * rp * 4);
    const ConvPlanes pl{xr.f(), xi.f(), yr.f(), yi.f(), tx, ty, rp};
    std::vector<ConvRowIO> io(nrows);
    for (int r = 0; r < nrows; r++) io[r] = ConvRowIO{dx.f((size_t)X.off[r] + (size_t)done * kBlock), out.f(r * rowlen + (size_t)done * kBlock)};
    DevIn<ConvRowIO> dio(io);
    launch_plane_copy(nullptr, pl.xr, tx, 0, c ? hR.f() : nullptr, hist, 0, hist, rp);
    launch_plane_copy(nullptr, pl.xi, tx, 0, c ? hI.f() : nullptr, hist, 0, hist, rp);
    const int tail = std::min(tx - (hist + n), 256);
    launch_plane_copy(nullptr, pl.xr, tx, hist + n, nullptr, 0, 0, tail, rp);
    launch_plane_copy(nullptr, pl.xi, tx, hist + n, nullptr, 0, 0, tail, rp);
    launch_rfft_fwd(nullptr, dio.p, nrows, n, hist, pl, gTw);
    launch_spectral_mac_shared(nullptr, pl, hr.f(), hi.f(), P, n, nrows);
    launch_irfft_ola(nullptr, dio.p, nrows, n, pl, ovs[c], ovs[c + 1], gTw);
    launch_plane_copy(nullptr, hR.f(), hist, 0, pl.xr, tx, n, hist, rp);
    launch_plane_copy(nullptr, hI.f(), hist, 0, pl.xi, tx, n, hist, rp);
    sync_check();
    dmg += xr.guard_damage() + xi.guard_damage() + yr.guard_damage() + yi.guard_damage();
    done += n;
  }
  dmg += out.guard_damage() + hR.guard_damage() + hI.guard_damage() + ov1.guard_damage() + ov2.guard_damage() + hr.guard_damage() + hi.guard_damage();
  chain_report(name, out.host((size_t)nrows * rowlen), want, dmg);
}
static void family_chain() {
  const Signals H = make_signals(1, kChainP, 0xC4A10001u, false);
  const Signals X = make_signals(3, kChainBlocks, 0xC4A10002u, false);
  GuardedIn dh(H.buf), dx(X.buf);
  const std::vector<float> taps(H.row(0), H.row(0) + (size_t)kChainP * kBlock);
  const size_t rowlen = (size_t)kChainBlocks * kBlock;
  std::vector<double> want;
  for (int r = 0; r < 3; r++) {
    const std::vector<double> w = direct_convolution(X.row(r), rowlen, taps);
    want.insert(want.end(), w.begin(), w.end());
  }
  Signals X0 = X;   // the B path convolves row 0
  X0.nrows = 1;
  const std::vector<double> want0(want.begin(), want.begin() + (long)rowlen);
  chain_b(false, X0, dx, H, dh, want0);
  chain_b(true, X0, dx, H, dh, want0);
  chain_a(X, dx, H, dh, want);
}

int main(int argc, char** argv) {
  const std::string fam = argc > 1 ? argv[1] : "";
  const auto t0 = std::chrono::steady_clock::now();
  if (fam != "fwd" && fam != "inv" && fam != "exact" && fam != "seam" && fam != "chain") {
    std::printf("usage: rfft_ref_check fwd|inv|exact|seam|chain\n");
    return 2;
  }
  TwTables tables;
  gTw = tables.tw;
  if (fam == "fwd") family_fwd();
  else if (fam == "inv") family_inv();
  else if (fam == "exact") family_exact();
  else if (fam == "seam") family_seam();
  else family_chain();
  std::printf("time %s %.2f s\n", fam.c_str(), std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  if (failures) std::printf("%d checks failed\n", failures);
  return failures ? 1 : 0;
}
