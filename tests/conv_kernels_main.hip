// Stand-alone run of the fine-partition convolver kernels of graphaudio_amd/csrc/ga_conv.hip through their launchers alone, against
// tests/conv_ref.hpp.  argv[1] picks a family:
//   a     spectral_mac_shared_kernel (formulation A) on integer spectra: bit for bit
//   b     spectral_mac_b_kernel (B) on integer spectra: bit for bit
//   r_int refmac_kernel (R) on integer spectra: equal to float64 and to B's output on the same tables
//   r_f32 refmac_kernel on uniform spectra: equal to the float32 reference-order loop bit for bit; one case with subnormal products
//   tap   tap_spectra_kernel<1024|2048|4096> against the float64 DFT, a derived bound
//   c     tconv_kernel / tconv16_kernel <1024|2048|4096> against the float64 linear convolution, a derived bound
//   util  hist_copy_b, plane_copy, extract_ir, pair_sum, stale_copy: exact
// Integer spectra are X and H in [-15, 15]: with the three-multiplication product the largest partial sum is 900 P < 2^24 for every P
// used here, so float32 in any order, with fma or on the matrix cores, equals float64 and the comparison is ==.
// Every output array lies between two guard regions filled with the byte 0xCD like the array itself: the guards must be untouched
// afterwards, no element the contract says is written may still read 0xCD, and every element it says is not written must.  Input arrays
// lie between guard regions of NaN, and every input element the contract says is not read is NaN: one NaN in a checked output means the
// kernel read outside what the planner prepares.  The tables are made the way ga_plan_conv.cpp makes them and are checked against the
// launchers' preconditions before anything is launched; a case outside them is reported and not run.
// Each check prints one line, "check <name> ok|FAIL <figures>", each launch of a templated kernel one line "instance <name>"; the
// program exits with status 1 if any check fails, and at once with status 3 after a HIP error (the caller then starts nothing more).
// (tests/test_gpu_conv_kernels.py runs the families and holds the set of check names and of instance names.)
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
#include "conv_ref.hpp"

using namespace ga;
namespace cv = conv_ref;
static_assert(cv::kBins == kBins, "tests/conv_ref.hpp restates the bin count");

namespace ga {
[[noreturn]] void launch_fail(const char* what) {   // (ga_engine.cpp's is not linked here)
  std::printf("launch_fail: %s\n", what);
  std::exit(2);
}
}  // namespace ga

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); std::fflush(stdout); std::exit(3); } } while (0)

static int failures = 0;
static void check(const std::string& name, bool ok, const char* fmt, ...) {
  char buf[512];
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
static void instance(const char* name) {
  std::printf("instance %s\n", name);
  std::fflush(stdout);
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
  float small_int() { return (float)((int)(next() % 31) - 15); }                          // integer in [-15, 15]
};
enum Fill { kInteger, kUniform, kTiny };   // kTiny: uniform x 2^-70 (products around 2^-140: subnormal)
static float draw(Rng& r, Fill f) {
  if (f == kInteger) return r.small_int();
  const float v = r.unit();
  return f == kTiny ? v * 8.470329472543003e-22f : v;
}

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
    CK(hipMemsetD32((hipDeviceptr_t)raw, (int)word, (g + bytes + g) / 4));
  }
  ~Guarded() { (void)hipFree(raw); }
  Guarded(const Guarded&) = delete;
  Guarded& operator=(const Guarded&) = delete;
  template <class T>
  T* ptr(size_t byte_off = 0) const { return (T*)(raw + g + byte_off); }
  void upload(const void* src, size_t n) { CK(hipMemcpy(raw + g, src, n, hipMemcpyHostToDevice)); }
  std::vector<float> host(size_t nfloats) const {
    std::vector<float> h(nfloats);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h.data(), raw + g, nfloats * 4, hipMemcpyDeviceToHost));
    return h;
  }
  size_t guard_damage() const {   // words of the guards (and of the round-up behind the array) that no longer hold `word`
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

// ---- twiddle tables: the formulas of Context::twiddlesC and Context::twiddles16 (ga_engine.cpp) ---------------------------------------
static std::vector<float2> twiddlesC(int N2) {
  const double pi = 3.14159265358979323846264338327950288;
  std::vector<float2> t(N2);
  for (int j = 0; j < N2; j++) t[j] = make_float2((float)std::cos(2.0 * pi * j / N2), (float)-std::sin(2.0 * pi * j / N2));
  return t;
}
static std::vector<float2> twiddles16(int N2) {
  const double pi = 3.14159265358979323846264338327950288;
  std::vector<float2> t;
  for (int m = 1; m < 16; m++)
    for (int kk = 0; kk < 16; kk++) t.push_back(make_float2((float)std::cos(2.0 * pi * kk * m / 256), (float)-std::sin(2.0 * pi * kk * m / 256)));
  for (int m = 1; m < N2 / 256; m++)
    for (int j = 0; j < 256; j++) t.push_back(make_float2((float)std::cos(2.0 * pi * j * m / N2), (float)-std::sin(2.0 * pi * j * m / N2)));
  return t;
}

// =====================================================================================================================
//  a: the shared-IR multiply-accumulate.  Planes as the planner allocates them (planConvolversShared): ty = roundup(n, 64),
//  tx = ty + P + 128, history in rows [0, P - 1), the chunk behind it, then min(tx - (hist + n), 256) rows of zeros.  Since
//  tx - (hist + n) = ty - n + 129 <= 192, those rows always reach tx: no row inside a bin's plane is NaN, a read past tx of bins 0..127
//  lands in the next bin's (finite) history, and only a read past tx of bin 128 meets the NaN guard -- the [bin][block][row] layout
//  leaves room for no other canary; that the zeroed rows suffice is what the values say (a stale row would show).  Rows nrows .. rp hold finite junk (the planner's padding rows are zero or stale spectra).
// =====================================================================================================================
static void run_a(int rp, int nrows, int n, int P) {
  const std::string name = fmt("a.rp%d.r%d.n%d.P%d", rp, nrows, n, P);
  const int hist = P - 1, ty = roundup(n, 64), tx = ty + P + 128;
  const int nrt = (nrows + 127) / 128, tail = std::min(tx - (hist + n), 256);
  if (rp % 128 || nrt * 128 > rp || nrows < 1 || n < 1 || P < 1 || 900.0 * P >= 16777216.0) {
    check(name, false, "not run: outside the launcher's preconditions");
    return;
  }
  const size_t xsz = (size_t)kBins * tx * rp;
  std::unique_ptr<float[]> xr(new float[xsz]), xi(new float[xsz]);   // (filled below, a bin per thread)
  std::vector<float> hr((size_t)kBins * P), hi(hr.size());
  parallel_for(kBins, [&](size_t k) {
    Rng rng{0xA000u + (uint64_t)P * 131 + n * 7 + nrows + k * 7919};
    for (int t = 0; t < tx; t++)
      for (int r = 0; r < rp; r++) {
        const size_t o = (k * tx + t) * rp + r;
        const bool zero = t >= hist + n, nan = t >= hist + n + tail;
        xr[o] = nan ? kNaNf : (zero ? 0.f : rng.small_int());
        xi[o] = nan ? kNaNf : (zero ? 0.f : rng.small_int());
      }
    for (int p = 0; p < P; p++) {
      hr[k * P + p] = rng.small_int();
      hi[k * P + p] = rng.small_int();
    }
  });
  GuardedIn dxr(xr.get(), xsz), dxi(xi.get(), xsz), dhr(hr), dhi(hi);
  const size_t ysz = (size_t)kBins * ty * rp;
  Guarded dyr(ysz * 4), dyi(ysz * 4);
  ConvPlanes pl{dxr.ptr<float>(), dxi.ptr<float>(), dyr.ptr<float>(), dyi.ptr<float>(), tx, ty, rp};
  launch_spectral_mac_shared(nullptr, pl, dhr.ptr<float>(), dhi.ptr<float>(), P, n, nrows);
  sync_check();
  const std::vector<float> yr = dyr.host(ysz), yi = dyi.host(ysz);
  std::atomic<long> wrong{0}, nans{0}, stray{0}, unwritten{0};
  parallel_for(kBins, [&](size_t k) {
    std::vector<double> rr((size_t)ty * nrows), ri((size_t)ty * nrows);
    cv::mac_a_bin(xr.get() + k * tx * rp, xi.get() + k * tx * rp, rp, hr.data() + k * P, hi.data() + k * P, P, ty, nrows, rr.data(), ri.data());
    long w = 0, nn = 0, st = 0, un = 0;
    for (int t = 0; t < ty; t++)
      for (int r = 0; r < rp; r++) {
        const float gr = yr[(k * ty + t) * rp + r], gi = yi[(k * ty + t) * rp + r];
        if (r < nrows) {
          nn += (gr != gr) + (gi != gi);
          un += is_cd(gr) + is_cd(gi);
          w += ((double)gr != rr[(size_t)t * nrows + r]) + ((double)gi != ri[(size_t)t * nrows + r]);
        } else if (r >= nrt * 128) {
          st += !is_cd(gr) + !is_cd(gi);
        }
      }
    wrong += w; nans += nn; stray += st; unwritten += un;
  });
  const size_t dmg = dyr.guard_damage() + dyi.guard_damage();
  check(name, !wrong && !nans && !stray && !unwritten && !dmg, "wrong %ld nan %ld unwritten %ld stray %ld guard %zu (ty %d tx %d zero rows %d)",
        wrong.load(), nans.load(), unwritten.load(), stray.load(), dmg, ty, tx, tail);
}
static void family_a() {
  // tile totals 129 x ntt x nrt are never a multiple of 8 here (ntt, nrt in {1, 2, 3}): the L >= total tail of the XCD map runs
  for (int P : {1, 2, 15, 16, 17, 64, 65})
    for (int n : {1, 63, 64, 65, 130})
      for (int nrows : {1, 128, 129}) run_a(nrows > 128 ? 256 : 128, nrows, n, P);
  for (int n : {1, 65}) run_a(256, 1, n, 17);   // a row tile of the planes the launch does not cover: it stays 0xCD
  for (int P : {1024, 1025})                    // the second tap segment; few rows, so that the host reference stays short
    for (int n : {1, 65, 130}) run_a(128, n == 130 ? 3 : 1, n, P);
}

// =====================================================================================================================
//  b, r, c: the [row][bin][block] layout.  Planes as the planner's PrivateStage lays them out: tx = hist + roundup(n, 16) + 16,
//  ty = roundup(n, 256); X holds values in [0, hist + n) and NaN behind; sets with x and y0 out of order.
// =====================================================================================================================
struct SetSpec { int x, y0, ncol; };
struct Problem {
  int P, n, hist, tx, ty, nx, ny, ncols;
  std::vector<SetSpec> sets;
  std::vector<int> col0;           // first column (index into h) of every set
  std::vector<float> xr, xi;       // [nx][kBins][tx]
  std::vector<float> hr, hi;       // [ncols][kBins][P]
  const float* xrow(const std::vector<float>& x, int row, int k) const { return x.data() + ((size_t)row * kBins + k) * tx; }
  const float* hcol(const std::vector<float>& h, int c, int k) const { return h.data() + ((size_t)c * kBins + k) * P; }
};
static Problem make_problem(int P, int n, int hist, const std::vector<SetSpec>& sets, int nx, int ny, Fill fill, uint64_t seed) {
  Problem q;
  q.P = P; q.n = n; q.hist = hist; q.nx = nx; q.ny = ny; q.sets = sets;
  q.tx = hist + roundup(n, 16) + 16;
  q.ty = roundup(n, 256);
  q.ncols = 0;
  for (const SetSpec& s : sets) {
    q.col0.push_back(q.ncols);
    q.ncols += s.ncol;
  }
  Rng rng{seed};
  q.xr.assign((size_t)nx * kBins * q.tx, kNaNf);
  q.xi.assign(q.xr.size(), kNaNf);
  for (int row = 0; row < nx * kBins; row++)
    for (int i = 0; i < hist + n; i++) {
      q.xr[(size_t)row * q.tx + i] = draw(rng, fill);
      q.xi[(size_t)row * q.tx + i] = draw(rng, fill);
    }
  q.hr.resize((size_t)q.ncols * kBins * P);
  q.hi.resize(q.hr.size());
  for (float& v : q.hr) v = draw(rng, fill);
  for (float& v : q.hi) v = draw(rng, fill);
  return q;
}
// what the launchers take for granted; nullptr: fine
static const char* outside_contract(const Problem& q) {
  if (q.P < 1 || q.n < 1 || q.hist < 0 || q.hist % 4) return "P, n or hist";
  if (q.tx < q.hist + q.n || q.ty < roundup(q.n, 4) || q.ty % 4) return "plane extents";
  std::vector<int> owner(q.ny, -1);
  for (size_t s = 0; s < q.sets.size(); s++) {
    const SetSpec& S = q.sets[s];
    if (S.ncol < 1 || S.ncol > 16 || S.x < 0 || S.x >= q.nx || S.y0 < 0 || S.y0 + S.ncol > q.ny) return "a set outside the planes";
    for (int j = 0; j < S.ncol; j++) {
      if (owner[S.y0 + j] >= 0) return "two sets share a y row";
      owner[S.y0 + j] = (int)s;
    }
  }
  return nullptr;
}
// the sets b and r share: ncol = 1, 2, 15 and 16 in one launch; y rows 0-2, 19, 23 and 39 belong to no set
static const std::vector<SetSpec> kSetsB = {{2, 20, 1}, {0, 3, 16}, {1, 21, 2}, {0, 24, 15}};
constexpr int kNxB = 3, kNyB = 40;

struct DeviceProblem {
  GuardedIn xr, xi, hr, hi;
  explicit DeviceProblem(const Problem& q) : xr(q.xr), xi(q.xi), hr(q.hr), hi(q.hi) {}
  std::vector<ConvSetB> setsB(const Problem& q) const {
    std::vector<ConvSetB> v;
    for (size_t s = 0; s < q.sets.size(); s++) {
      ConvSetB S{};
      S.x = q.sets[s].x; S.y0 = q.sets[s].y0; S.ncol = q.sets[s].ncol; S.P = q.P;
      for (int j = 0; j < S.ncol; j++) {
        S.hr[j] = hr.ptr<float>() + (size_t)(q.col0[s] + j) * kBins * q.P;
        S.hi[j] = hi.ptr<float>() + (size_t)(q.col0[s] + j) * kBins * q.P;
      }
      v.push_back(S);
    }
    return v;
  }
};
struct YPlanes {
  Guarded yr, yi;
  size_t n;
  explicit YPlanes(const Problem& q) : yr((size_t)q.ny * kBins * q.ty * 4), yi((size_t)q.ny * kBins * q.ty * 4), n((size_t)q.ny * kBins * q.ty) {}
  ConvPlanesB planes(const Problem& q, const DeviceProblem& d) { return ConvPlanesB{d.xr.ptr<float>(), d.xi.ptr<float>(), yr.ptr<float>(), yi.ptr<float>(), q.tx, q.ty}; }
};

// float64 reference of every column: [ncols][kBins][nt]
struct Ref64 { std::vector<double> re, im; int nt; };
static Ref64 reference64(const Problem& q, int nt) {
  Ref64 R;
  R.nt = nt;
  R.re.resize((size_t)q.ncols * kBins * nt);
  R.im.resize(R.re.size());
  std::vector<int> colx(q.ncols);
  for (size_t s = 0; s < q.sets.size(); s++)
    for (int j = 0; j < q.sets[s].ncol; j++) colx[q.col0[s] + j] = q.sets[s].x;
  parallel_for((size_t)q.ncols * kBins, [&](size_t i) {
    const int c = (int)(i / kBins), k = (int)(i % kBins);
    cv::linconv(q.xrow(q.xr, colx[c], k), q.xrow(q.xi, colx[c], k), q.hist, q.n, q.hcol(q.hr, c, k), q.hcol(q.hi, c, k), q.P, nt, R.re.data() + i * nt,
                R.im.data() + i * nt);
  });
  return R;
}
struct Ref32 { std::vector<float> re, im; int nt; };
static Ref32 reference32(const Problem& q, int nt) {
  Ref32 R;
  R.nt = nt;
  R.re.resize((size_t)q.ncols * kBins * nt);
  R.im.resize(R.re.size());
  std::vector<int> colx(q.ncols);
  for (size_t s = 0; s < q.sets.size(); s++)
    for (int j = 0; j < q.sets[s].ncol; j++) colx[q.col0[s] + j] = q.sets[s].x;
  parallel_for((size_t)q.ncols * kBins, [&](size_t i) {
    const int c = (int)(i / kBins), k = (int)(i % kBins);
    cv::refmac_f32(q.xrow(q.xr, colx[c], k), q.xrow(q.xi, colx[c], k), q.hist, q.n, q.hcol(q.hr, c, k), q.hcol(q.hi, c, k), q.P, nt, R.re.data() + i * nt,
                   R.im.data() + i * nt);
  });
  return R;
}

// Walks every element of the y planes.  An element of a set's column with block index in [w0, w1) must be written: match(c, k, t, re,
// im) says whether it is right.  Every other element must still read 0xCD.
struct Tally { long wrong = 0, nan = 0, unwritten = 0, stray = 0; bool clean() const { return !wrong && !nan && !unwritten && !stray; } };
template <class M>
static Tally walk(const Problem& q, const std::vector<float>& yr, const std::vector<float>& yi, int w0, int w1, M match) {
  std::vector<int> ycol(q.ny, -1);
  for (size_t s = 0; s < q.sets.size(); s++)
    for (int j = 0; j < q.sets[s].ncol; j++) ycol[q.sets[s].y0 + j] = q.col0[s] + j;
  std::vector<Tally> part(q.ny);
  parallel_for(q.ny, [&](size_t row) {
    Tally T;
    const int c = ycol[row];
    for (int k = 0; k < kBins; k++)
      for (int t = 0; t < q.ty; t++) {
        const float gr = yr[(row * kBins + k) * q.ty + t], gi = yi[(row * kBins + k) * q.ty + t];
        if (c >= 0 && t >= w0 && t < w1) {
          T.nan += (gr != gr) + (gi != gi);
          T.unwritten += is_cd(gr) + is_cd(gi);
          T.wrong += !match(c, k, t, gr, gi);
        } else {
          T.stray += !is_cd(gr) + !is_cd(gi);
        }
      }
    part[row] = T;
  });
  Tally T;
  for (const Tally& p : part) { T.wrong += p.wrong; T.nan += p.nan; T.unwritten += p.unwritten; T.stray += p.stray; }
  return T;
}
static void report(const std::string& name, const Tally& T, size_t dmg, const char* extra = "") {
  check(name, T.clean() && !dmg, "wrong %ld nan %ld unwritten %ld stray %ld guard %zu %s", T.wrong, T.nan, T.unwritten, T.stray, dmg, extra);
}
static int hist_of(int P, char h) { return h == '0' ? 0 : roundup(P - 1, 4) + (h == 'g' ? 8 : 0); }   // none, as the planner, greater

// b: every block of [0, ty) of every set column is written (the store guard is t < ty), X = 0 from block n on
static void run_b(int P, int n, char h) {
  const std::string name = fmt("b.P%d.n%d.h%c", P, n, h);
  const Problem q = make_problem(P, n, hist_of(P, h), kSetsB, kNxB, kNyB, kInteger, 0xB000u + (uint64_t)P * 977 + n * 13 + h);
  if (const char* why = outside_contract(q)) { check(name, false, "not run: %s", why); return; }
  if (q.ty != roundup(n, 256)) { check(name, false, "not run: ty"); return; }
  DeviceProblem d(q);
  YPlanes y(q);
  DevIn<ConvSetB> sets(d.setsB(q));
  launch_spectral_mac_b(nullptr, sets.p, (int)q.sets.size(), n, q.hist, y.planes(q, d));
  sync_check();
  const std::vector<float> yr = y.yr.host(y.n), yi = y.yi.host(y.n);
  const Ref64 R = reference64(q, q.ty);
  const Tally T = walk(q, yr, yi, 0, q.ty, [&](int c, int k, int t, float gr, float gi) {
    const size_t o = ((size_t)c * kBins + k) * R.nt + t;
    return (double)gr == R.re[o] && (double)gi == R.im[o];
  });
  report(name, T, y.yr.guard_damage() + y.yi.guard_damage());
}
static const int kPb[] = {1, 3, 4, 5, 255, 256, 257, 600};          // Ps4 padding; 1, 2 and 3 tap segments of 256
static const int kNb[] = {1, 3, 255, 256, 257, 520};                // 1, 2 and 3 time tiles of 256
static void family_b() {
  for (int P : kPb)
    for (int n : kNb) run_b(P, n, 'r');
  for (int P : kPb)
    for (int n : {3, 257})
      for (char h : {'0', 'g'}) run_b(P, n, h);
}

// r: blocks [0, roundup(n, 4)) are written (a lane stores its quad when its first block is < n); the rest of the row stays 0xCD
static void run_r(int P, int n, char h, Fill fill) {
  const char* mode = fill == kInteger ? "int" : (fill == kUniform ? "f32" : "tiny");
  const std::string name = fmt("r.%s.P%d.n%d.h%c", mode, P, n, h);
  const Problem q = make_problem(P, n, hist_of(P, h), kSetsB, kNxB, kNyB, fill, 0xC000u + (uint64_t)P * 977 + n * 13 + h + fill);
  if (const char* why = outside_contract(q)) { check(name, false, "not run: %s", why); return; }
  DeviceProblem d(q);
  YPlanes y(q);
  DevIn<ConvSetB> sets(d.setsB(q));
  launch_refmac(nullptr, sets.p, (int)q.sets.size(), n, q.hist, y.planes(q, d));
  sync_check();
  const std::vector<float> yr = y.yr.host(y.n), yi = y.yi.host(y.n);
  const int n4 = roundup(n, 4);
  if (fill == kInteger) {   // (i) equal to float64, and to formulation B on the same tables
    YPlanes yb(q);
    launch_spectral_mac_b(nullptr, sets.p, (int)q.sets.size(), n, q.hist, yb.planes(q, d));
    sync_check();
    const std::vector<float> br = yb.yr.host(yb.n), bi = yb.yi.host(yb.n);
    const Ref64 R = reference64(q, n4);
    std::vector<int> yrow(q.ncols);
    for (size_t s = 0; s < q.sets.size(); s++)
      for (int j = 0; j < q.sets[s].ncol; j++) yrow[q.col0[s] + j] = q.sets[s].y0 + j;
    std::atomic<long> vsb{0};
    const Tally T = walk(q, yr, yi, 0, n4, [&](int c, int k, int t, float gr, float gi) {
      const size_t o = ((size_t)c * kBins + k) * R.nt + t, ob = ((size_t)yrow[c] * kBins + k) * q.ty + t;
      if (bits(gr) != bits(br[ob]) && gr != br[ob]) vsb++;
      if (bits(gi) != bits(bi[ob]) && gi != bi[ob]) vsb++;
      return (double)gr == R.re[o] && (double)gi == R.im[o];
    });
    const size_t dmg = y.yr.guard_damage() + y.yi.guard_damage();
    check(name, T.clean() && !dmg && !vsb, "wrong %ld nan %ld unwritten %ld stray %ld guard %zu differs from B %ld", T.wrong, T.nan, T.unwritten,
          T.stray, dmg, vsb.load());
  } else {                  // (ii), (iii) equal to the float32 reference-order loop bit for bit, the sign of zero included
    const Ref32 R = reference32(q, n4);
    long nonzero = 0, subnormal = 0;
    for (float v : R.re) {
      nonzero += v != 0.f;
      subnormal += v != 0.f && std::fabs(v) < 1.17549435e-38f;
    }
    const Tally T = walk(q, yr, yi, 0, n4, [&](int c, int k, int t, float gr, float gi) {
      const size_t o = ((size_t)c * kBins + k) * R.nt + t;
      return bits(gr) == bits(R.re[o]) && bits(gi) == bits(R.im[o]);
    });
    // (the case means something only if the reference itself holds such values)
    const bool meaningful = fill == kTiny ? subnormal > 0 : nonzero > 0;
    const size_t dmg = y.yr.guard_damage() + y.yi.guard_damage();
    check(name, T.clean() && !dmg && meaningful, "wrong %ld nan %ld unwritten %ld stray %ld guard %zu nonzero %ld subnormal %ld", T.wrong, T.nan,
          T.unwritten, T.stray, dmg, nonzero, subnormal);
  }
}
// r_int and r_f32 run the same shapes: all 80 of b, both ends of the second tap segment and of the second time tile of 1024, and both
// at once.  (Two process runs, so that each stays at a few seconds: the host sums are the cost.)
static void family_r(Fill f) {
  for (int P : kPb)
    for (int n : kNb) run_r(P, n, 'r', f);
  for (int P : kPb)
    for (int n : {3, 257})
      for (char h : {'0', 'g'}) run_r(P, n, h, f);
  for (int P : {1023, 1024, 1025, 1030}) run_r(P, 5, 'r', f);   // the second tap segment
  for (int n : {1023, 1024, 1025, 1028}) run_r(5, n, 'r', f);   // the second time tile
  run_r(257, 1025, 'r', f);
  run_r(1030, 1028, 'r', f);
  if (f == kUniform) run_r(257, 257, 'r', kTiny);   // (iii) products around 2^-140: the reference's x86 arithmetic keeps subnormals
}

// =====================================================================================================================
//  Derived bounds of the float families (u = 2^-24, gamma_k = k u / (1 - k u); Higham, Accuracy and Stability of Numerical Algorithms).
//  Theorem 24.2: a radix-2 Cooley-Tukey transform of N = 2^t points whose twiddles carry errors of at most mu satisfies
//    ||computed - exact||_2 <= (t eta / (1 - t eta)) ||exact||_2,   eta = mu + gamma_4 (sqrt 2 + mu);
//  the tables here are correctly rounded double-precision values, mu = u.  The Stockham radix-8 / radix-4 passes and the radix-16
//  passes evaluate the same butterflies with fewer intermediate roundings (and fma in the twiddle products).
//   tap:  per (channel, bin)  || hs N2 - DFT ||_2 <= t eta ||DFT||_2   (the scaling by 1 / N2 is exact)
//   c:    per (set, column, bin, segment), x = the segment's window of N2 blocks, X = F x exact (||X||_2 = sqrt N ||x||_2),
//         g = DFT(h) / N exact, y = F'(X o g) the circular convolution whose last N - P + 1 elements are the linear one.  Computed:
//           X~ = X + d1,            ||d1||_2 <= e ||X||_2,           e = t eta / (1 - t eta)            (forward transform)
//           g~ = g + d2,            ||d2||_2 <= e ||g||_2 <= e sqrt N max|g|  -- a norm bound, so per bin only |d2_j| <= e sqrt N max|g|
//           p~_j = X~_j g~_j (1 + eps_j),  |eps_j| <= sqrt 2 gamma_2                                    (Lemma 3.5, complex product)
//         With ||a o b||_2 <= ||a||_2 max|b|:  ||p~ - X o g||_2 <= ||X||_2 max|g| (A - 1),  ||p~||_2 <= ||X||_2 max|g| A,
//           A = (1 + e)(1 + e sqrt N)(1 + sqrt 2 gamma_2).
//         The inverse transform (conjugation or swap: exact) adds ||d3||_2 <= e sqrt N ||p~||_2, and F' scales norms by sqrt N:
//           ||y~ - y||_2 <= sqrt N ||X||_2 max|g| ((1 + e) A - 1) = c(N) ||x||_2 max_j |DFT(h)_j|,   c(N) = (1 + e) A - 1.
//         The error over the valid blocks is at most the error over all N.  c(1024) = 1.4e-4, c(2048) = 2.1e-4, c(4096) = 3.2e-4;
//         the sqrt N comes from knowing the taps' spectrum only in norm.  A one-block shift, a dropped column or a wrong segment is of
//         order ||y|| >= ||x|| max|DFT(h)| / sqrt P on this scale: 0.03 at P = 1024.
// =====================================================================================================================
static const double kU = 5.9604644775390625e-08;
static double gamma_k(double k) { return k * kU / (1.0 - k * kU); }
static double eta() { return kU + gamma_k(4) * (std::sqrt(2.0) + kU); }
static double bound_tap(int N2) { return std::log2((double)N2) * eta(); }
static double bound_c(int N2) {
  const double te = std::log2((double)N2) * eta(), e = te / (1.0 - te);
  const double A = (1.0 + e) * (1.0 + e * std::sqrt((double)N2)) * (1.0 + std::sqrt(2.0) * gamma_k(2));
  return (1.0 + e) * A - 1.0;
}

static void run_tap(int N2, int P, int nch) {
  const std::string name = fmt("tap.N%d.P%d.c%d", N2, P, nch);
  if (P < 1 || P > N2 || nch < 1) { check(name, false, "not run: outside the launcher's preconditions"); return; }
  std::vector<float> hr((size_t)nch * kBins * P), hi(hr.size());
  Rng rng{0xD000u + (uint64_t)N2 + P * 31 + nch};
  for (float& v : hr) v = rng.unit();
  for (float& v : hi) v = rng.unit();
  GuardedIn dhr(hr), dhi(hi);
  DevIn<float2> tw(twiddlesC(N2));
  const size_t nout = (size_t)nch * kBins * N2 * 2;
  Guarded hs(nout * 4);
  instance(launch_tap_spectra(nullptr, hs.ptr<float2>(), dhr.ptr<float>(), dhi.ptr<float>(), nch, P, N2, tw.p));
  sync_check();
  const std::vector<float> got = hs.host(nout);
  std::vector<double> ratio((size_t)nch * kBins, 0.0);
  std::atomic<long> unwritten{0};
  const double bound = bound_tap(N2);
  parallel_for((size_t)nch * kBins, [&](size_t i) {
    const std::vector<cv::cd> ref = cv::tap_spectrum(hr.data() + i * P, hi.data() + i * P, P, N2);
    double e2 = 0.0, n2 = 0.0;
    long un = 0;
    for (int j = 0; j < N2; j++) {
      const float a = got[(i * N2 + j) * 2], b = got[(i * N2 + j) * 2 + 1];
      un += is_cd(a) + is_cd(b);
      const double dr = (double)a * N2 - ref[j].re, di = (double)b * N2 - ref[j].im;
      e2 += dr * dr + di * di;
      n2 += ref[j].re * ref[j].re + ref[j].im * ref[j].im;
    }
    unwritten += un;
    const double r = std::sqrt(e2) / (bound * std::sqrt(n2));
    ratio[i] = r == r ? r : 1e300;
  });
  const double worst = *std::max_element(ratio.begin(), ratio.end());
  const size_t dmg = hs.guard_damage();
  check(name, worst <= 1.0 && !unwritten && !dmg, "ratio %.4f of the bound %.3e, unwritten %ld guard %zu", worst, bound, unwritten.load(), dmg);
}
static void family_tap() {
  for (int N2 : {1024, 2048, 4096})
    for (int P : {1, 65, N2 / 4, N2 / 4 + 1})
      for (int nch : {1, 3}) run_tap(N2, P, nch);
}

// ---- c ----------------------------------------------------------------------------------------------------------------
struct Launch { int N2, tbase, nseg; };
struct CCase {
  std::string name;
  int P, n, hist;
  std::vector<SetSpec> sets;
  int nx, ny;
  std::vector<Launch> plan;   // launches of tconv16 that together cover what `covered` says
  bool radix8;                // also through launch_tconv (one launch: plan.size() == 1, tbase == 0)
  bool radix16;
  uint64_t seed;
};
// per (column, bin, segment of the launch): the l2 error over the segment's valid blocks against c(N2) ||window||_2 max|DFT(h)|
static double worst_ratio_c(const Problem& q, const Ref64& R, const std::vector<float>& yr, const std::vector<float>& yi, const Launch& L) {
  const int seglen = L.N2 - (q.P - 1);
  std::vector<int> colx(q.ncols), yrow(q.ncols);
  for (size_t s = 0; s < q.sets.size(); s++)
    for (int j = 0; j < q.sets[s].ncol; j++) {
      colx[q.col0[s] + j] = q.sets[s].x;
      yrow[q.col0[s] + j] = q.sets[s].y0 + j;
    }
  std::vector<double> worst((size_t)q.ncols * kBins, 0.0);
  const double cN = bound_c(L.N2);
  parallel_for((size_t)q.ncols * kBins, [&](size_t i) {
    const int c = (int)(i / kBins), k = (int)(i % kBins);
    const std::vector<cv::cd> H = cv::tap_spectrum(q.hcol(q.hr, c, k), q.hcol(q.hi, c, k), q.P, L.N2);
    double hmax = 0.0;
    for (const cv::cd& v : H) hmax = std::max(hmax, std::hypot(v.re, v.im));
    const float* xr = q.xrow(q.xr, colx[c], k);
    const float* xi = q.xrow(q.xi, colx[c], k);
    for (int seg = 0; seg < L.nseg; seg++) {
      const int t0 = L.tbase + seg * seglen;
      if (t0 >= q.n) break;
      double w2 = 0.0, e2 = 0.0;
      for (int e = 0; e < L.N2; e++) {
        const int blk = t0 - (q.P - 1) + e;
        if (blk >= -q.hist && blk < q.n) w2 += (double)xr[q.hist + blk] * xr[q.hist + blk] + (double)xi[q.hist + blk] * xi[q.hist + blk];
      }
      for (int t = t0; t < std::min(q.n, t0 + seglen); t++) {
        const size_t o = ((size_t)yrow[c] * kBins + k) * q.ty + t, orf = i * R.nt + t;
        const double dr = yr[o] - R.re[orf], di = yi[o] - R.im[orf];
        e2 += dr * dr + di * di;
      }
      const double r = std::sqrt(e2) / (cN * std::sqrt(w2) * hmax);
      worst[i] = std::max(worst[i], r == r ? r : 1e300);
    }
  });
  return *std::max_element(worst.begin(), worst.end());
}
static void run_c(const CCase& C) {
  const Problem q = make_problem(C.P, C.n, C.hist, C.sets, C.nx, C.ny, kUniform, C.seed);
  const char* why = outside_contract(q);
  for (const Launch& L : C.plan)
    if (!why && (L.N2 - (C.P - 1) < 1 || L.tbase < 0 || L.nseg < 1)) why = "segment length or base";
  if (!why && C.radix8 && (C.plan.size() != 1 || C.plan[0].tbase != 0 || C.plan[0].nseg * (C.plan[0].N2 - (C.P - 1)) < C.n)) why = "launch_tconv covers the chunk from block 0";
  if (why) { check(C.name, false, "not run: %s", why); return; }
  DeviceProblem d(q);
  const Ref64 R = reference64(q, q.n);
  // the taps' spectra of every length the plan uses, by the library's own kernel
  std::vector<int> lens;
  for (const Launch& L : C.plan)
    if (std::find(lens.begin(), lens.end(), L.N2) == lens.end()) lens.push_back(L.N2);
  std::vector<std::unique_ptr<Guarded>> hs;
  for (int N2 : lens) {
    DevIn<float2> tw(twiddlesC(N2));
    hs.emplace_back(new Guarded((size_t)q.ncols * kBins * N2 * 8));
    instance(launch_tap_spectra(nullptr, hs.back()->ptr<float2>(), d.hr.ptr<float>(), d.hi.ptr<float>(), q.ncols, q.P, N2, tw.p));
    sync_check();
  }
  auto setsC = [&](int N2) {
    const float2* base = hs[std::find(lens.begin(), lens.end(), N2) - lens.begin()]->ptr<float2>();
    std::vector<ConvSetC> v;
    for (size_t s = 0; s < q.sets.size(); s++) {
      ConvSetC S{};
      S.x = q.sets[s].x; S.y0 = q.sets[s].y0; S.ncol = q.sets[s].ncol; S.P = q.P;
      for (int j = 0; j < S.ncol; j++) S.hs[j] = base + (size_t)(q.col0[s] + j) * kBins * N2;
      v.push_back(S);
    }
    return v;
  };
  auto judge = [&](const std::string& name, YPlanes& y, const Launch& L) {
    const std::vector<float> yr = y.yr.host(y.n), yi = y.yi.host(y.n);
    const int w0 = L.tbase, w1 = std::min(q.n, L.tbase + L.nseg * (L.N2 - (q.P - 1)));
    const Tally T = walk(q, yr, yi, w0, w1, [&](int, int, int, float, float) { return true; });   // (values: the bound below)
    const double ratio = T.clean() ? worst_ratio_c(q, R, yr, yi, L) : -1.0;
    const size_t dmg = y.yr.guard_damage() + y.yi.guard_damage();
    check(name, T.clean() && !dmg && ratio >= 0.0 && ratio <= 1.0, "ratio %.5f of the bound (c = %.3e), blocks [%d, %d): nan %ld unwritten %ld stray %ld guard %zu",
          ratio, bound_c(L.N2), w0, w1, T.nan, T.unwritten, T.stray, dmg);
  };
  if (C.radix8) {
    const Launch& L = C.plan[0];
    DevIn<float2> tw(twiddlesC(L.N2));
    DevIn<ConvSetC> sets(setsC(L.N2));
    YPlanes y(q);
    instance(launch_tconv(nullptr, sets.p, (int)q.sets.size(), q.n, q.hist, y.planes(q, d), L.N2, tw.p, L.nseg));
    sync_check();
    judge(C.name + ".r8", y, L);
  }
  if (C.radix16) {
    if (!tconv16_hist_ok(q.hist, q.P)) {   // the radix-16 kernel has no guard in front of -hist: refused, not launched
      check(C.name + ".r16_refused", true, "hist %d < P - 1 = %d: launch_tconv16 is not called", q.hist, q.P - 1);
      return;
    }
    // every launch of the plan into planes of its own: each writes its own blocks and no others, together they write [0, n) once
    std::vector<char> cover(q.n, 0);
    bool once = true;
    for (size_t l = 0; l < C.plan.size(); l++) {
      const Launch& L = C.plan[l];
      DevIn<float2> tw(twiddles16(L.N2));
      DevIn<ConvSetC> sets(setsC(L.N2));
      YPlanes y(q);
      instance(launch_tconv16(nullptr, sets.p, (int)q.sets.size(), q.n, q.hist, y.planes(q, d), L.N2, tw.p, L.nseg, L.tbase));
      sync_check();
      judge(C.name + (C.plan.size() > 1 ? fmt(".r16.launch%zu", l) : std::string(".r16")), y, L);
      for (int t = L.tbase; t < std::min(q.n, L.tbase + L.nseg * (L.N2 - (q.P - 1))); t++) once = once && !cover[t]++;
    }
    if (C.plan.size() > 1) {
      for (char cvd : cover) once = once && cvd == 1;
      check(C.name + ".r16.once", once, "every block of [0, %d) belongs to exactly one launch", q.n);
    }
  }
}
static void family_c() {
  const std::vector<SetSpec> s3 = {{1, 4, 1}, {0, 6, 16}, {1, 0, 3}};   // ncol 1, 16 and 3 share a step at G = 4; y rows 3, 5, 22 are free
  const std::vector<SetSpec> s2 = {{1, 4, 3}, {0, 1, 1}};               // y rows 0, 2, 3, 7 are free
  auto h = [](int P) { return roundup(P - 1, 4); };
  std::vector<CCase> cases = {
      // N2 = 1024 (L = 960 at P = 65, 768 at P = 257); G = 4: 3, 6, 15 items leave idle transforms in the last step
      {"c.1024.P65.s1", 65, 959, h(65), s3, 2, 23, {{1024, 0, 1}}, true, true},      // n < L, nvalid = L - 1
      {"c.1024.P65.s2", 65, 961, h(65), s3, 2, 23, {{1024, 0, 2}}, true, true},      // nvalid = 1
      {"c.1024.P257.s2", 257, 769, h(257), s3, 2, 23, {{1024, 0, 2}}, true, true},   // nvalid = 1
      {"c.1024.P257.s5", 257, 3839, h(257), s3, 2, 23, {{1024, 0, 5}}, true, true},  // nvalid = L - 1
      {"c.1024.tbase", 65, 1065, h(65), s3, 2, 23, {{1024, 100, 2}}, false, true},   // blocks [0, 100) stay 0xCD
      {"c.1024.hist0", 65, 500, 0, s3, 2, 23, {{1024, 0, 1}}, true, true},           // radix 8 only: its guard allows hist = 0
      // N2 = 2048 (L = 1920 at P = 129, 1537 at P = 512); G = 2
      {"c.2048.P129.s2", 129, 1921, h(129), s3, 2, 23, {{2048, 0, 2}}, true, true},  // nvalid = 1
      {"c.2048.P512.s1", 512, 1536, h(512), s2, 2, 8, {{2048, 0, 1}}, true, true},   // n < L, nvalid = L - 1
      {"c.2048.tbase", 129, 1000, h(129), s2, 2, 8, {{2048, 64, 1}}, false, true},
      // N2 = 4096 (L = 3585 at P = 512, 3073 at P = 1024); G = 1
      {"c.4096.P512.s2", 512, 3586, h(512), s2, 2, 8, {{4096, 0, 2}}, true, true},   // nvalid = 1
      {"c.4096.P1024.s1", 1024, 3072, h(1024), s2, 2, 8, {{4096, 0, 1}}, true, true},// n < L, nvalid = L - 1
      {"c.4096.tbase", 512, 2000, h(512), s2, 2, 8, {{4096, 513, 1}}, false, true},
      // Context::tconvPlan(3750, 512): one segment of 4096 points, then one of 1024 at tbase = 3585
      {"c.mixed", 512, 3750, h(512), s2, 2, 8, {{4096, 0, 1}, {1024, 3585, 1}}, false, true},
  };
  for (size_t i = 0; i < cases.size(); i++) cases[i].seed = 0xE000u + 31 * i;   // (fixed inputs per case)
  for (const CCase& C : cases) run_c(C);
}

// =====================================================================================================================
//  util
// =====================================================================================================================
static std::vector<float> floats(size_t n, uint64_t seed) {
  Rng r{seed};
  std::vector<float> v(n);
  for (float& x : v) x = r.unit();
  return v;
}
static void util_hist_copy() {
  // one launch: n = 1, 63, 64, 65 with a source, n = 0, and n = 40 without a source; strides unequal; all 129 bins (the 33rd group of
  // four has one live wave)
  struct J { int n, ds, ss; bool src; };
  const J js[6] = {{1, 5, 3, true}, {63, 70, 64, true}, {64, 64, 80, true}, {65, 81, 66, true}, {0, 8, 8, true}, {40, 47, 0, false}};
  std::vector<std::unique_ptr<Guarded>> dst;
  std::vector<std::unique_ptr<GuardedIn>> src;
  std::vector<std::vector<float>> hsrc;
  std::vector<HistJobB> jobs;
  int max_n = 0;
  for (int i = 0; i < 6; i++) {
    hsrc.push_back(floats((size_t)kBins * std::max(1, js[i].ss), 0xF00 + i));
    src.emplace_back(new GuardedIn(hsrc.back()));
    dst.emplace_back(new Guarded((size_t)kBins * js[i].ds * 4));
    jobs.push_back(HistJobB{dst.back()->ptr<float>(), js[i].src ? src.back()->ptr<float>() : nullptr, js[i].ds, js[i].ss, js[i].n, 0});
    max_n = std::max(max_n, js[i].n);
  }
  DevIn<HistJobB> dj(jobs);
  launch_hist_copy_b(nullptr, dj.p, 6, max_n);
  sync_check();
  long bad = 0;
  size_t dmg = 0;
  for (int i = 0; i < 6; i++) {
    const size_t nd = (size_t)kBins * js[i].ds;
    const std::vector<float> got = dst[i]->host(nd);
    std::vector<float> want(nd, from_bits(kCD));
    cv::hist_copy_b(cv::HistJob{want.data(), js[i].src ? hsrc[i].data() : nullptr, js[i].ds, js[i].ss, js[i].n});
    for (size_t e = 0; e < nd; e++) bad += bits(got[e]) != bits(want[e]);
    dmg += dst[i]->guard_damage();
  }
  check("util.hist_copy_b", !bad && !dmg, "wrong %ld guard %zu", bad, dmg);
}
static void util_plane_copy() {
  struct PC { const char* name; int dst_t, dst_t0, src_t, src_t0, n, rp; bool src; };
  // the last one: n rp / 4 = 131,200 float4 per bin, above the 512 x 256 threads of the capped grid, which then strides
  const PC cs[3] = {{"util.plane_copy.offset", 7, 2, 5, 1, 3, 128, true}, {"util.plane_copy.null", 6, 1, 0, 0, 4, 256, false},
                    {"util.plane_copy.strided", 2052, 1, 2051, 1, 2050, 256, true}};
  for (const PC& c : cs) {
    const size_t nd = (size_t)kBins * c.dst_t * c.rp, ns = (size_t)kBins * std::max(1, c.src_t) * c.rp;
    std::vector<float> hsrc(ns);
    for (size_t i = 0; i < ns; i++) hsrc[i] = (float)(int)((i * 2654435761u) >> 12 & 0xFFFFF);   // (cheap, distinct enough)
    GuardedIn src(hsrc);
    Guarded dst(nd * 4);
    if ((size_t)c.n * c.rp % 4 || c.dst_t0 + c.n > c.dst_t || (c.src && c.src_t0 + c.n > c.src_t)) { check(c.name, false, "not run: outside the planes"); continue; }
    launch_plane_copy(nullptr, dst.ptr<float>(), c.dst_t, c.dst_t0, c.src ? src.ptr<float>() : nullptr, c.src_t, c.src_t0, c.n, c.rp);
    sync_check();
    const std::vector<float> got = dst.host(nd);
    std::vector<float> want(nd, from_bits(kCD));
    cv::plane_copy(want.data(), c.dst_t, c.dst_t0, c.src ? hsrc.data() : nullptr, c.src_t, c.src_t0, c.n, c.rp);
    long bad = 0;
    for (size_t e = 0; e < nd; e++) bad += bits(got[e]) != bits(want[e]);
    const size_t dmg = dst.guard_damage();
    check(c.name, !bad && !dmg, "wrong %ld guard %zu", bad, dmg);
  }
}
static void util_extract_ir() {
  for (int nch : {1, 3}) {
    const int P = nch == 1 ? 3 : 5, tx = P + 2, rp = 128;   // totals 387 and 1935: no multiple of 256
    const std::vector<float> xr = floats((size_t)kBins * tx * rp, 0xF10 + nch), xi = floats(xr.size(), 0xF20 + nch);
    GuardedIn dxr(xr), dxi(xi);
    const size_t nh = (size_t)nch * kBins * P;
    Guarded hr(nh * 4), hi(nh * 4);
    launch_extract_ir(nullptr, hr.ptr<float>(), hi.ptr<float>(), dxr.ptr<float>(), dxi.ptr<float>(), tx, rp, P, nch);
    sync_check();
    // (the arrays are rounded up to 256 bytes: the words behind nh must still read 0xCD)
    const std::vector<float> gr = hr.host(hr.bytes / 4), gi = hi.host(hi.bytes / 4);
    std::vector<float> wr(hr.bytes / 4, from_bits(kCD)), wi(wr);
    cv::extract_ir(wr.data(), xr.data(), tx, rp, P, nch);
    cv::extract_ir(wi.data(), xi.data(), tx, rp, P, nch);
    long bad = 0;
    for (size_t e = 0; e < wr.size(); e++) bad += (bits(gr[e]) != bits(wr[e])) + (bits(gi[e]) != bits(wi[e]));
    const size_t dmg = hr.guard_damage() + hi.guard_damage();
    check(fmt("util.extract_ir.c%d", nch), !bad && !dmg, "wrong %ld guard %zu", bad, dmg);
  }
}
static void util_pair_sum() {
  for (int64_t n : {(int64_t)1, (int64_t)255, (int64_t)256, (int64_t)4096 * 256 + 77}) {   // the last: above the grid cap of 4096 x 256
    const std::vector<float> a = floats((size_t)n, 0xF30 + n), b = floats((size_t)n, 0xF40 + n);
    GuardedIn da(a), db(b);
    Guarded out((size_t)n * 4);
    launch_pair_sum(nullptr, out.ptr<float>(), da.ptr<float>(), db.ptr<float>(), n);
    sync_check();
    const std::vector<float> got = out.host(out.bytes / 4);
    std::vector<float> want(out.bytes / 4, from_bits(kCD));
    cv::pair_sum(want.data(), a.data(), b.data(), n);
    long bad = 0;
    for (size_t e = 0; e < want.size(); e++) bad += bits(got[e]) != bits(want[e]);
    const size_t dmg = out.guard_damage();
    check(fmt("util.pair_sum.n%lld", (long long)n), !bad && !dmg, "wrong %ld guard %zu", bad, dmg);
  }
}
static void util_stale_copy() {
  const std::vector<float> a = floats(128, 0xF50), c = floats(128, 0xF51);
  GuardedIn da(a), dc(c);
  Guarded out(4 * 128 * 4);   // four rows; the last one belongs to no job
  std::vector<StaleJob> jobs(3);
  jobs[0].dst = out.ptr<float>() + 256; jobs[0].src = da.ptr<float>(); jobs[0].scale = 0.3f;
  jobs[1].dst = out.ptr<float>(); jobs[1].src = da.ptr<float>(); jobs[1].scale = 0.3f; jobs[1].curve = dc.ptr<float>();
  jobs[2].dst = out.ptr<float>() + 128; jobs[2].src = nullptr; jobs[2].scale = 0.3f; jobs[2].curve = dc.ptr<float>();
  DevIn<StaleJob> dj(jobs);
  launch_stale_copy(nullptr, dj.p, 3);
  sync_check();
  const std::vector<float> got = out.host(512);
  std::vector<float> want(512, from_bits(kCD));
  cv::stale_copy(want.data() + 256, a.data(), 0.3f, nullptr);
  cv::stale_copy(want.data(), a.data(), 0.3f, c.data());
  cv::stale_copy(want.data() + 128, nullptr, 0.3f, c.data());
  long bad = 0;
  for (int e = 0; e < 512; e++) bad += bits(got[e]) != bits(want[e]);
  const size_t dmg = out.guard_damage();
  check("util.stale_copy", !bad && !dmg, "wrong %ld guard %zu", bad, dmg);
}
static void family_util() {
  util_hist_copy();
  util_plane_copy();
  util_extract_ir();
  util_pair_sum();
  util_stale_copy();
}

int main(int argc, char** argv) {
  const std::string fam = argc > 1 ? argv[1] : "";
  const auto t0 = std::chrono::steady_clock::now();
  if (fam == "a") family_a();
  else if (fam == "b") family_b();
  else if (fam == "r_int") family_r(kInteger);
  else if (fam == "r_f32") family_r(kUniform);
  else if (fam == "tap") family_tap();
  else if (fam == "c") family_c();
  else if (fam == "util") family_util();
  else {
    std::printf("usage: conv_kernels_check a|b|r_int|r_f32|tap|c|util\n");
    return 2;
  }
  std::printf("time %s %.2f s\n", fam.c_str(), std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  if (failures) std::printf("%d checks failed\n", failures);
  return failures ? 1 : 0;
}
