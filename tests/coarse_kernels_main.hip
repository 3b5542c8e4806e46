// Stand-alone run of the kernels of graphaudio_amd/csrc/ga_coarse.hip (formulation D of the convolver) through their launchers alone,
// instance by instance, against the float64 reference tests/coarse_ref.hpp.  argv[1] picks a family:
//   mac        every instance launch_coarse_mac can dispatch to, on integer spectra: bit for bit (every product and partial sum is an
//              integer below 2^24, so float32 in any order, with fma or MFMA, equals float64), and the returned instance name
//   mac_float  one case each of mac, sum, seg and mfma16 on uniform spectra, against a derived bound
//   fwd, inv   the transforms: exact identities, and a derived bound on the relative l2 error per window / block
//   premix     the compensated time-domain sum: exact on integers, Kahan's bound on uniform inputs, independent of the grid
//   hist       the history copy: exact
//   chain      forward (taps and signal), multiply-accumulate, inverse against direct float64 convolution
// Every output array lies between two guard regions filled with the byte 0xCD like the array itself: the guards must be untouched
// afterwards, no element the contract says is written may still read 0xCD, and every element it says is not written must.
// Each check prints one line, "check <name> ok|FAIL <figures>"; the program exits nonzero if any check fails.
// (tests/test_gpu_coarse_kernels.py runs the families and holds the set of check names and of instance names.)
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "ga_kernels.hpp"
#include "coarse_ref.hpp"

using namespace ga;
namespace cr = coarse_ref;
static_assert(cr::CB == kCoarseBlock && cr::NB == kCoarseBins, "tests/coarse_ref.hpp restates the two constants");

namespace ga {
[[noreturn]] void launch_fail(const char* what) {   // (ga_engine.cpp's is not linked here)
  std::printf("launch_fail: %s\n", what);
  std::exit(2);
}
}  // namespace ga

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); std::exit(1); } } while (0)

constexpr int CB = kCoarseBlock, NB = kCoarseBins;
using cf = cr::Cx<float>;
using cd = cr::cd;

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
  float unit() { return (float)((double)(int64_t)(next() >> 40) / 8388608.0 - 1.0); }   // 24 bits -> [-1, 1), exact
  float small_int() { return (float)((int)(next() % 31) - 15); }                          // integer in [-15, 15]
};
static void fill(std::vector<float>& v, uint64_t seed, bool integer) {
  Rng r{seed};
  for (float& x : v) x = integer ? r.small_int() : r.unit();
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

constexpr uint32_t kCD = 0xCDCDCDCDu;
static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
static bool is_cd(float f) { return bits(f) == kCD; }
static float cd_float() {
  float f;
  const uint32_t u = kCD;
  std::memcpy(&f, &u, 4);
  return f;
}

// device array between two guard regions; everything starts as the byte 0xCD
struct Guarded {
  char* raw = nullptr;
  size_t bytes, gf, gb;
  explicit Guarded(size_t bytes_, size_t gf_ = 65536, size_t gb_ = 65536) : bytes((bytes_ + 255) / 256 * 256), gf(gf_), gb(gb_) {
    CK(hipMalloc(&raw, gf + bytes + gb));
    CK(hipMemset(raw, 0xCD, gf + bytes + gb));
  }
  ~Guarded() { (void)hipFree(raw); }
  Guarded(const Guarded&) = delete;
  Guarded& operator=(const Guarded&) = delete;
  template <class T>
  T* ptr(size_t byte_off = 0) const { return (T*)(raw + gf + byte_off); }
  void upload(const void* src, size_t n, size_t byte_off = 0) { CK(hipMemcpy(raw + gf + byte_off, src, n, hipMemcpyHostToDevice)); }
  std::vector<float> host(size_t nfloats) const {
    std::vector<float> h(nfloats);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h.data(), raw + gf, nfloats * 4, hipMemcpyDeviceToHost));
    return h;
  }
  size_t guard_damage() const {   // bytes of the guards that no longer read 0xCD
    CK(hipDeviceSynchronize());
    size_t bad = 0;
    std::vector<unsigned char> g(std::max(gf, gb));
    CK(hipMemcpy(g.data(), raw, gf, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < gf; i++) bad += g[i] != 0xCD;
    CK(hipMemcpy(g.data(), raw + gf + bytes, gb, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < gb; i++) bad += g[i] != 0xCD;
    return bad;
  }
};
template <class T>
struct DevIn {   // plain device input
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

// ---- twiddle tables: the formulas of Context::twiddles16, Context::twiddles16pw and Context::coarseTwab (ga_engine.cpp) ----------
static std::vector<float2> twiddles16(int N2) {
  const double pi = 3.14159265358979323846264338327950288;
  std::vector<float2> t;
  for (int m = 1; m < 16; m++)
    for (int kk = 0; kk < 16; kk++) t.push_back(make_float2((float)std::cos(2.0 * pi * kk * m / 256), (float)-std::sin(2.0 * pi * kk * m / 256)));
  for (int m = 1; m < N2 / 256; m++)
    for (int j = 0; j < 256; j++) t.push_back(make_float2((float)std::cos(2.0 * pi * j * m / N2), (float)-std::sin(2.0 * pi * j * m / N2)));
  return t;
}
static std::vector<float2> twiddles16pw() {
  const double pi = 3.14159265358979323846264338327950288;
  std::vector<float2> t;
  for (int m = 1; m < 16; m++)
    for (int kk = 0; kk < 16; kk++) t.push_back(make_float2((float)std::cos(2.0 * pi * kk * m / 256), (float)-std::sin(2.0 * pi * kk * m / 256)));
  for (int m : {1, 2, 4, 8})
    for (int j = 0; j < 256; j++) t.push_back(make_float2((float)std::cos(2.0 * pi * j * m / 4096), (float)-std::sin(2.0 * pi * j * m / 4096)));
  return t;
}
static std::vector<float2> coarse_twab() {
  const double pi = 3.14159265358979323846264338327950288;
  std::vector<float2> t(2 * 2049);
  for (int k = 0; k <= 2048; k++) {
    t[k] = make_float2((float)std::cos(2.0 * pi * k / 8192), (float)-std::sin(2.0 * pi * k / 8192));
    t[2049 + k] = make_float2((float)std::cos(2.0 * pi * k / 16384), (float)-std::sin(2.0 * pi * k / 16384));
  }
  return t;
}
struct Tables {
  DevIn<float2> inv{twiddles16(4096)}, fwd{twiddles16pw()}, ab{coarse_twab()};
};

// =====================================================================================================================
//  multiply-accumulate
// =====================================================================================================================
struct Sig { int u_first, nwin, frame0; };       // a transformed signal: frames of the windows [u_first, u_first + nwin)
struct Ir { int P, Pstore; size_t off; };        // spectra [cw][Pstore][NB] at float2 offset `off` (rows >= P: zero rows)
struct JobSpec {
  int P, t0, n_t, u_lo, u_hi, shared, yrow0;
  std::vector<int> sig, ir;                      // per term
};
struct MacCase {
  std::string name, expect;
  int cw = 1, pb = 1;
  bool any_private = true, mfma = false;
  std::vector<Sig> sigs;
  std::vector<Ir> irs;
  std::vector<JobSpec> jobs;
  int frames = 0, yrows = 0;
  size_t hsize = 0;
  int add_sig(int u_first, int nwin) {
    sigs.push_back(Sig{u_first, nwin, frames});
    frames += nwin;
    return (int)sigs.size() - 1;
  }
  int add_ir(int P) {
    const int Ps = P > kCoarseMaxP ? (P + kCoarseMaxP - 1) / kCoarseMaxP * kCoarseMaxP : P;   // (Context::ensureCoarseSpectra: whole segments)
    irs.push_back(Ir{P, Ps, hsize});
    hsize += (size_t)cw * Ps * NB;
    return (int)irs.size() - 1;
  }
  // a job over signals (and impulse responses) of its own: the signals hold exactly the windows [u_lo, u_hi]
  void add_job(int P, int t0, int n_t, int u_lo, int u_hi, int nterms, bool shared) {
    JobSpec j{P, t0, n_t, u_lo, u_hi, shared ? 1 : 0, yrows, {}, {}};
    const int one = shared ? add_ir(P) : -1;
    for (int i = 0; i < nterms; i++) {
      j.sig.push_back(add_sig(u_lo, u_hi - u_lo + 1));
      j.ir.push_back(shared ? one : add_ir(P));
    }
    yrows += cw;
    jobs.push_back(j);
  }
  // a job over the first `nterms` of the signals [sig0, ...) and one impulse response, all made before
  void add_shared_job(int P, int t0, int n_t, int u_lo, int u_hi, int sig0, int nterms, int ir) {
    JobSpec j{P, t0, n_t, u_lo, u_hi, 1, yrows, {}, {}};
    for (int i = 0; i < nterms; i++) {
      j.sig.push_back(sig0 + i);
      j.ir.push_back(ir);
    }
    yrows += cw;
    jobs.push_back(j);
  }
};

static std::set<std::string> gInstances;
static bool gDry = false;   // argv[2] = "dry": the multiply-accumulate cases are checked against the contracts and listed, nothing is launched

// exact: integer spectra, bit for bit.  Otherwise uniform spectra and, per element,
//   |got - ref| <= gamma sum |X| |H|,   gamma = (n + 2) 2^-24 sqrt(2),   n = products accumulated into the element:
// a float32 complex product carries a relative error of at most sqrt(2) gamma_2 (Higham, Accuracy and Stability, Lemma 3.5), a sum
// of n such products in any order at most gamma_(n-1) more on the sum of the moduli (section 3.1), together sqrt(2) gamma_(n+2), and
// gamma_k = k u / (1 - k u) ~ k 2^-24.  Fused multiply-adds and the matrix cores round less often; the reduction kernel adds the terms'
// frames first (terms - 1 roundings) and multiplies once per partition: terms + P <= n + 1 roundings.  Position 0 holds two real
// inner products: the same bound without the sqrt(2), per real.  (Derived, not measured; the largest ratio observed is printed.)
// the launchers' contracts as the planner keeps them, checked before anything is launched: a case outside them is a mistake of this
// program and is reported, not run
static const char* outside_contract(const MacCase& C) {
  bool seg = false;
  for (const JobSpec& j : C.jobs) seg = seg || j.P > kCoarseMaxP;
  for (const JobSpec& j : C.jobs) {
    if (j.n_t < 1 || j.n_t > (C.any_private ? kCoarseJobBlocks(C.cw) : kCoarseSumJobBlocks(C.cw))) return "n_t beyond the job size";
    if (j.P < 1 || j.P > kCoarseMaxParts || (C.cw == 16 && j.P > kCoarseMaxP)) return "partition count";
    if (!seg && C.any_private && j.P % C.pb) return "P is no multiple of pb";
    if (j.sig.empty() || (int)j.sig.size() > kCoarseJobTerms) return "terms per job";
    if (!C.any_private && !j.shared) return "a private job in a reduction launch";
    for (size_t i = 0; i < j.sig.size(); i++) {
      const Sig& s = C.sigs[j.sig[i]];
      const int lo = std::max(j.u_lo, j.t0 - (j.P - 1)), hi = std::min(j.u_hi, j.t0 + j.n_t - 1);
      if (lo <= hi && (lo < s.u_first || hi >= s.u_first + s.nwin)) return "a window that exists lies outside the signal's frames";
      if (C.irs[j.ir[i]].P != j.P) return "impulse response of another length";
      if (j.shared && j.ir[i] != j.ir[0]) return "shared_h with different spectra";
    }
  }
  return nullptr;
}

static void run_mac_case(const MacCase& C, bool exact) {
  if (const char* why = outside_contract(C)) {
    check(C.name, false, "not run: %s", why);
    return;
  }
  if (gDry) {
    std::printf("dry %s: %zu jobs, %d frames, expects %s\n", C.name.c_str(), C.jobs.size(), C.frames, C.expect.c_str());
    return;
  }
  const bool seg = [&] { for (const JobSpec& j : C.jobs) if (j.P > kCoarseMaxP) return true; return false; }();
  std::vector<float> X((size_t)C.frames * NB * 2), H(C.hsize * 2, 0.f);
  fill(X, 0x1000 + std::hash<std::string>{}(C.name) % 997, exact);
  {
    Rng r{0x2000 + C.name.size()};
    for (const Ir& ir : C.irs)
      for (int c = 0; c < C.cw; c++)
        for (int p = 0; p < ir.P; p++) {
          float* row = H.data() + 2 * (ir.off + ((size_t)c * ir.Pstore + p) * NB);
          for (int i = 0; i < 2 * NB; i++) row[i] = exact ? r.small_int() : r.unit();
        }
  }
  // frames in front of the first row are guard: a term's frame0 may point there (windows that do not exist), and a fetch from there
  // would put -4.3e8 into a sum
  const size_t xguard = (size_t)(kCoarseMaxParts + 2 * kCoarseMaxP) * NB * sizeof(float2);
  Guarded dX(X.size() * 4, xguard, 65536), dH(H.size() * 4);
  dX.upload(X.data(), X.size() * 4);
  dH.upload(H.data(), H.size() * 4);
  const float2* Xd = dX.ptr<float2>();
  const float2* Hd = dH.ptr<float2>();
  int y_frames = 0, max_t = 0, maxP = 0;
  for (const JobSpec& j : C.jobs) {
    y_frames = std::max(y_frames, j.t0 + j.n_t + 1);
    max_t = std::max(max_t, j.n_t);
    maxP = std::max(maxP, j.P);
  }
  // the device tables, as CoarseStage::buildJobs (ga_plan_conv.cpp) makes them
  std::vector<CoarseTerm> terms;
  std::vector<CoarseJob> jobs;
  auto hptr = [&](const Ir& ir, int c, int off) { return Hd + ir.off + ((size_t)c * ir.Pstore + off) * NB; };
  // (a few unused terms in front: term0 > 0 for every job)
  for (int i = 0; i < 3; i++) {
    CoarseTerm t{};
    t.frame0 = 1 << 20;
    terms.push_back(t);
  }
  for (const JobSpec& j : C.jobs) {
    CoarseJob J{};
    J.term0 = (int)terms.size();
    J.P = j.P;
    J.t0 = j.t0;
    J.n_t = j.n_t;
    J.yrow0 = j.yrow0;
    J.shared_h = j.shared;
    J.u_lo = j.u_lo;
    J.u_hi = j.u_hi;
    const bool jseg = seg && j.P > kCoarseMaxP;
    for (size_t i = 0; i < j.sig.size(); i++) {
      const Sig& s = C.sigs[j.sig[i]];
      const Ir& ir = C.irs[j.ir[i]];
      const int frame_u0 = s.frame0 - s.u_first;   // frame the window u = 0 has (or would have)
      if (!jseg) {
        CoarseTerm t{};
        t.frame0 = frame_u0 - (j.P - 1);           // frame of the window u = -(P - 1)
        for (int c = 0; c < C.cw; c++) t.h[c] = hptr(ir, c, 0);
        terms.push_back(t);
      } else if (!C.any_private) {                 // reduction kernel: frame of the window u = 0; the kernel walks the segments itself
        CoarseTerm t{};
        t.frame0 = frame_u0;
        for (int c = 0; c < C.cw; c++) t.h[c] = hptr(ir, c, 0);
        terms.push_back(t);
      } else {                                     // general kernel: (signal, segment) pairs; segments none of whose windows exist are left out
        for (int off = 0; off < j.P; off += kCoarseMaxP) {
          const int np = std::min(kCoarseMaxP, (j.P - off + 3) / 4 * 4);
          const int wLo = std::max(j.u_lo, j.t0 - off - (kCoarseMaxP - 1)), wHi = std::min(j.u_hi, j.t0 + j.n_t - 1 - off);
          if (wLo > wHi || j.t0 - off - (np - 1) > j.u_hi) continue;
          CoarseTerm t{};
          t.frame0 = frame_u0 - off - (kCoarseMaxP - 1);
          t.pad_ = off + 256 * np;
          for (int c = 0; c < C.cw; c++) t.h[c] = hptr(ir, c, off);
          terms.push_back(t);
        }
      }
    }
    J.n_terms = (int)terms.size() - J.term0;
    if (J.n_terms <= 0) { check(C.name, false, "the case makes a job without terms"); return; }
    jobs.push_back(J);
  }
  DevIn<CoarseTerm> dT(terms);
  DevIn<CoarseJob> dJ(jobs);
  const size_t ny = (size_t)C.yrows * y_frames * NB * 2;
  Guarded dY(ny * 4);
  const char* name = launch_coarse_mac(0, dJ.p, (int)jobs.size(), dT.p, Xd, dY.ptr<float2>(), y_frames, C.cw, max_t, maxP, C.any_private, C.pb, C.mfma);
  sync_check();
  gInstances.insert(name);
  std::printf("instance %s\n", name);
  const std::vector<float> got = dY.host(ny);
  const size_t damage = dY.guard_damage();

  // the reference, one (job, column, block) per work item; blocks no job covers stay 0xCD
  struct Item { int j, c, t; };
  std::vector<Item> items;
  for (size_t j = 0; j < C.jobs.size(); j++)
    for (int c = 0; c < C.cw; c++)
      for (int t = 0; t < C.jobs[j].n_t; t++) items.push_back(Item{(int)j, c, t});
  std::vector<char> covered((size_t)C.yrows * y_frames, 0);
  std::atomic<size_t> bad{0}, bad0{0}, zsign{0};
  std::vector<double> ratio(items.size(), 0.0);
  parallel_for(items.size(), [&](size_t k) {
    const Item it = items[k];
    const JobSpec& j = C.jobs[it.j];
    cr::MacJob<float> J;
    J.P = j.P;
    J.t0 = j.t0;
    J.n_t = j.n_t;
    J.u_lo = j.u_lo;
    J.u_hi = j.u_hi;
    for (size_t i = 0; i < j.sig.size(); i++) {
      const Sig& s = C.sigs[j.sig[i]];
      const Ir& ir = C.irs[j.ir[i]];
      cr::MacTerm<float> t{(const cf*)X.data(), s.frame0 - s.u_first, {}};
      for (int c = 0; c < C.cw; c++) t.h[c] = (const cf*)H.data() + ir.off + (size_t)c * ir.Pstore * NB;
      J.terms.push_back(t);
    }
    std::vector<cd> y(NB);
    std::vector<double> mag(exact ? 0 : 2 * NB);
    int n = 0;
    cr::ref_mac(J, it.c, it.t, y.data(), exact ? nullptr : mag.data(), &n);
    const size_t row = (size_t)(j.yrow0 + it.c) * y_frames + j.t0 + it.t;
    covered[row] = 1;
    const float* g = got.data() + row * NB * 2;
    size_t b = 0, b0 = 0, zs = 0;
    if (exact) {
      for (int i = 0; i < NB; i++) {
        const float wr = (float)y[i].re, wi = (float)y[i].im;
        const bool same = bits(g[2 * i]) == bits(wr) && bits(g[2 * i + 1]) == bits(wi);
        const bool same_value = g[2 * i] == wr && g[2 * i + 1] == wi && !is_cd(g[2 * i]) && !is_cd(g[2 * i + 1]);
        if (!same && same_value) zs++;   // (a zero of the other sign)
        if (!same_value) {
          b++;
          if (i == 0) b0++;
        }
      }
    } else {
      const double u = std::ldexp(1.0, -24), gam = (n + 2) * u;
      double worst = 0.0;
      for (int i = 0; i < NB; i++) {
        if (is_cd(g[2 * i]) || is_cd(g[2 * i + 1])) { b++; continue; }
        const double er = (double)g[2 * i] - y[i].re, ei = (double)g[2 * i + 1] - y[i].im;
        auto over = [](double err, double bound) { return err == 0.0 ? 0.0 : err / bound; };   // (no products: the element is exactly zero)
        double q;
        if (i == 0) q = std::max(over(std::fabs(er), gam * mag[0]), over(std::fabs(ei), gam * mag[1]));
        else q = over(std::hypot(er, ei), gam * std::sqrt(2.0) * mag[2 * i]);
        worst = std::max(worst, q);
        if (!(q <= 1.0)) {
          b++;
          if (i == 0) b0++;
        }
      }
      ratio[k] = worst;
    }
    bad += b;
    bad0 += b0;
    zsign += zs;
  });
  size_t stray = 0;
  for (size_t row = 0; row < covered.size(); row++)
    if (!covered[row])
      for (int i = 0; i < 2 * NB; i++) stray += !is_cd(got[row * NB * 2 + i]);
  const bool named = C.expect == name;
  const double worst = items.empty() ? 0.0 : *std::max_element(ratio.begin(), ratio.end());
  check(C.name, named && !bad && !stray && !damage, "instance %s%s wrong %zu stray %zu guard %zu zero_sign %zu%s", name,
        named ? "" : (" (expected " + C.expect + ")").c_str(), bad.load(), stray, damage, zsign.load(),
        exact ? "" : (" max_ratio " + std::to_string(worst)).c_str());
  if (C.cw == 16) check(C.name + ".bin0", !bad0, "position 0 (two real bins, element-wise) wrong %zu", bad0.load());
}

static std::string mac_name(int cw, int tw, int pb, int wv) {
  return "coarse_mac_kernel<" + std::to_string(cw) + "," + std::to_string(tw) + "," + std::to_string(pb) + "," + std::to_string(wv) + ">";
}
// TW = 2: n_t = 1, 7, 16 in one launch of three jobs (+ a shared_h job inside the private launch); whatever pb
static MacCase case_tw2(int cw) {
  MacCase C;
  C.name = "mac.c" + std::to_string(cw) + ".tw2";
  C.cw = cw;
  C.pb = 1;
  C.expect = mac_name(cw, 2, 1, 8);
  C.add_job(3, 0, 1, 0, 0, 1, false);        // no history, no tail
  C.add_job(5, 0, 7, -4, 2, 2, false);       // a chunk of 2 blocks that carries its tail: u_hi = nT, blocks up to nT + P
  C.add_job(2, 3, 16, -1, 18, 5, false);     // t0 > 0
  C.add_job(4, 1, 5, 0, 5, 3, true);         // every term on the same spectra, inside a private launch
  return C;
}
// the wide sweeps of 1, 2 and 4 columns: two jobs of different n_t and P, so that NFA and maxP belong to different jobs
static MacCase case_tw(int cw, int tw, int pb, int P, int n_lo, int n_hi, int pb_inst) {
  MacCase C;
  C.name = "mac.c" + std::to_string(cw) + ".tw" + std::to_string(tw) + ".pb" + std::to_string(pb);
  C.cw = cw;
  C.pb = pb;
  C.expect = mac_name(cw, tw, pb_inst, 8);
  C.add_job(P, 0, n_lo, 0, n_lo - P, 2, false);                   // no history; a chunk of n_lo - P blocks with its tail
  C.add_job(pb == 4 ? 4 : 2, 5, n_hi, -(pb == 4 ? 3 : 1), 5 + n_hi - 1, pb == 1 ? 5 : 1, false);
  if (pb == 2) C.add_job(P, 0, n_hi, -(P - 1), n_hi - 1, 3, true);   // shared spectra inside a private launch
  return C;
}
static MacCase case_wide(bool mfma, int P) {
  MacCase C;
  C.name = mfma ? "mac.c16.mfma.p" + std::to_string(P) : "mac.c16.general";
  C.cw = 16;
  C.pb = 1;
  C.mfma = mfma;
  C.expect = mfma ? "coarse_mfma16_kernel" : mac_name(16, 3, 1, 12);
  C.add_job(P, 0, 1, 0, 0, 1, false);
  C.add_job(P, 2, 13, -(P - 1), 14, 2, false);
  C.add_job(P, 0, 32, 0, 32 - P, 5, false);   // no history, tail
  return C;
}
// reduction kernel: n_terms = 1, 4, 5 and kCoarseJobTerms over one pool of signals and one impulse response
static MacCase case_sum(int cw) {
  MacCase C;
  C.name = "mac.sum.c" + std::to_string(cw);
  C.cw = cw;
  C.any_private = false;
  C.pb = 4;
  C.expect = "coarse_sum_kernel<" + std::to_string(cw) + ">";
  const int nt = kCoarseSumJobBlocks(cw), P = 16;
  const int ir = C.add_ir(P), ir7 = C.add_ir(7);
  for (int i = 0; i < kCoarseJobTerms; i++) C.add_sig(-(P - 1), nt + P);   // windows -(P - 1) .. nt
  C.add_shared_job(P, 0, nt, -(P - 1), nt - 1, 0, 1, ir);
  C.add_shared_job(P, 0, nt, 0, nt - P, 3, 4, ir);                         // no history, tail
  C.add_shared_job(7, 3, 20, -6, 22, 7, 5, ir7);                           // another n_t and P, t0 > 0
  C.add_shared_job(P, 0, nt, -(P - 1), nt - 1, 0, kCoarseJobTerms, ir);
  return C;
}
// segmented sums: P = 17, 32, 33 and 128 in one launch.  tw = 0: the reduction kernel.
static MacCase case_seg(int cw, int tw) {
  MacCase C;
  C.cw = cw;
  C.pb = 4;
  C.any_private = tw != 0;
  const int n_hi = tw == 0 ? kCoarseSumJobBlocks(cw) : (tw == 2 ? 16 : 8 * tw), n_mid = tw == 0 ? 10 : (tw == 2 ? 7 : (tw == 9 ? 65 : 17));
  if (tw) {
    C.name = "mac.seg.c" + std::to_string(cw) + ".tw" + std::to_string(tw);
    C.expect = "coarse_mac_seg_kernel<" + std::to_string(cw) + "," + std::to_string(tw) + ",4>";
  } else {
    C.name = "mac.sumseg.c" + std::to_string(cw);
    C.expect = "coarse_sum_seg_kernel<" + std::to_string(cw) + ">";
  }
  const bool sh = tw == 0;
  C.add_job(17, 0, n_hi, -16, n_hi - 1, 2, sh);
  // no history: the second segment of the first blocks has no window that exists (left out of the pairs / skipped by the reduction
  // kernel), and frame0 lies in front of the row
  C.add_job(32, tw == 0 ? 0 : 4, n_mid, 0, (tw == 0 ? 0 : 4) + n_mid - 1, sh ? 3 : 1, sh);
  C.add_job(33, 2, n_mid, -32, n_mid - 3, 2, sh);                // t0 > 0; the last four blocks lie behind u_hi (a carried tail)
  C.add_job(128, 0, n_mid, -127, n_mid - 1, sh ? 5 : 1, sh);
  return C;
}

static void family_mac() {
  for (int cw : {1, 2}) {
    run_mac_case(case_tw2(cw), true);
    for (int tw : {8, 9})
      for (int pb : {1, 2, 4}) run_mac_case(case_tw(cw, tw, pb, pb == 1 ? 3 : (pb == 2 ? 6 : 8), tw == 8 ? 17 : 65, tw == 8 ? 64 : 72, pb), true);
  }
  run_mac_case(case_tw2(4), true);
  run_mac_case(case_tw(4, 4, 1, 3, 17, 32, 1), true);
  run_mac_case(case_tw(4, 4, 4, 8, 17, 32, 2), true);   // pb 4 lands on PB = 2
  run_mac_case(case_wide(false, 5), true);
  run_mac_case(case_wide(true, 1), true);
  run_mac_case(case_wide(true, 4), true);
  for (int cw : {1, 2, 4}) run_mac_case(case_sum(cw), true);
  for (int cw : {1, 2}) for (int tw : {2, 8, 9}) run_mac_case(case_seg(cw, tw), true);
  for (int tw : {2, 4}) run_mac_case(case_seg(4, tw), true);
  for (int cw : {1, 2, 4}) run_mac_case(case_seg(cw, 0), true);
}
static void family_mac_float() {
  auto named = [](MacCase C, const char* name) { C.name = name; return C; };
  run_mac_case(named(case_tw(2, 8, 4, 8, 17, 64, 4), "mac_float.mac"), false);
  run_mac_case(named(case_sum(2), "mac_float.sum"), false);
  run_mac_case(named(case_seg(2, 8), "mac_float.seg"), false);
  run_mac_case(named(case_wide(true, 4), "mac_float.mfma16"), false);
}

// =====================================================================================================================
//  transforms
// =====================================================================================================================
// The bound of the two transform families, per window / block:  ||got - ref||_2 / ||ref||_2 <= 15 eta,  eta = u + 4 u (sqrt(2) + u),
// u = 2^-24: Higham, Accuracy and Stability, Theorem 24.2 -- a radix-2 transform of 2^t points with twiddles of relative error u
// has relative l2 error at most t eta / (1 - t eta) -- over the 14 stages of 16,384 points plus the combine pass (~ 6e-6).  The
// radix-16 transform rounds less often per point, so the bound is safe; one wrong block of 64 bins is ~ 1e-1.
constexpr double kU = 5.9604644775390625e-8;
static double transform_bound() { return 15.0 * (kU + 4.0 * kU * (std::sqrt(2.0) + kU)); }

struct Pool {   // host image of the sample buffers; offsets are 16-byte aligned unless `mis` floats are added
  std::vector<float> h;
  size_t take(size_t n, size_t mis = 0) {
    const size_t o = (h.size() + 3) / 4 * 4 + mis;
    h.resize(o + n + 4, 0.f);
    return o;
  }
};
struct RowSpec {
  long hist_off = -1, in_off = -1;
  int64_t nvalid = 0, hist_len = 0;
  int n_frames = 0, u0 = 0, flags = 0;
  float scale = 1.f;
  int frame0 = 0;
};
static cr::XRow host_row(const RowSpec& s, const Pool& p) {
  cr::XRow r;
  r.hist = s.hist_off >= 0 ? p.h.data() + s.hist_off : nullptr;
  r.in = s.in_off >= 0 ? p.h.data() + s.in_off : nullptr;
  r.nvalid = s.nvalid;
  r.n_frames = s.n_frames;
  r.u0 = s.u0;
  r.hist_len = s.hist_len;
  r.flags = s.flags;
  r.scale = s.scale;
  return r;
}
static CoarseXRow dev_row(const RowSpec& s, const float* dpool, float* carry = nullptr, int64_t carry_from = 0) {
  CoarseXRow r{};
  r.hist = s.hist_off >= 0 ? dpool + s.hist_off : nullptr;
  r.in = s.in_off >= 0 ? dpool + s.in_off : nullptr;
  r.nvalid = s.nvalid;
  r.frame0 = s.frame0;
  r.n_frames = s.n_frames;
  r.u0 = s.u0;
  r.hist_len = (int)s.hist_len;
  r.flags = s.flags;
  r.scale = s.scale;
  r.carry = carry;
  r.carry_from = carry_from;
  return r;
}
// one forward launch into a fresh guarded frame buffer
static std::vector<float> run_fwd(const Tables& T, const std::vector<CoarseXRow>& rows, int frames, int run, size_t* damage,
                                  const std::vector<CoarseHandOver>& ho = {}) {
  DevIn<CoarseXRow> dR(rows);
  DevIn<CoarseHandOver> dHo(ho);
  Guarded dX((size_t)frames * NB * 8);
  int max_frames = 0;
  for (const CoarseXRow& r : rows) max_frames = std::max(max_frames, r.n_frames);
  const char* name = launch_coarse_fwd(0, dR.p, (int)rows.size(), max_frames, run, dX.ptr<float2>(), T.fwd.p, T.ab.p, ho.empty() ? nullptr : dHo.p, (int)ho.size());
  sync_check();
  if (std::strcmp(name, "coarse_fwd_kernel")) check("fwd.instance", false, "launcher returned %s", name);
  *damage += dX.guard_damage();
  return dX.host((size_t)frames * NB * 2);
}
static size_t differing(const std::vector<float>& a, const std::vector<float>& b) {
  size_t n = a.size() != b.size();
  for (size_t i = 0; i < std::min(a.size(), b.size()); i++) n += bits(a[i]) != bits(b[i]);
  return n;
}

static void family_fwd() {
  Tables T;
  // ---- exact identities ----
  {
    Pool P;
    const int64_t hl = 2 * CB, nv = 4 * (int64_t)CB + 384;
    RowSpec A;
    A.hist_off = (long)P.take(hl);
    A.in_off = (long)P.take(nv);
    A.nvalid = nv;
    A.hist_len = hl;
    A.u0 = -1;
    A.n_frames = 7;
    RowSpec B = A;
    B.in_off = (long)P.take(nv, 1);   // the same samples, one float off 16-byte alignment
    fill(P.h, 11, false);
    std::memcpy(P.h.data() + B.in_off, P.h.data() + A.in_off, nv * 4);
    DevIn<float> dP(P.h);
    size_t damage = 0;
    const std::vector<float> x1 = run_fwd(T, {dev_row(A, dP.p)}, 7, 1, &damage);
    size_t d = 0;
    for (int run : {2, 5, 7}) d += differing(x1, run_fwd(T, {dev_row(A, dP.p)}, 7, run, &damage));
    size_t unwritten = 0;
    for (float v : x1) unwritten += is_cd(v);
    check("fwd.run_invariant", !d && !damage && !unwritten, "run 1 against 2, 5, n_frames: differ %zu unwritten %zu guard %zu", d, unwritten, damage);
    damage = 0;
    d = differing(x1, run_fwd(T, {dev_row(B, dP.p)}, 7, 2, &damage));
    check("fwd.unaligned_view", !d && !damage, "aligned against a view offset by one float: differ %zu guard %zu", d, damage);
    // carry[s - carry_from] = in[s], and a hand-over row to page-locked host memory in the same launch
    const int64_t cfrom = nv - hl, hn = 4 * (3 * 512 + 77);
    Guarded carry((size_t)hl * 4);
    float* pinned = nullptr;
    float* pinned_dev = nullptr;
    const size_t pg = 1024;   // guard floats on both sides of the host row
    CK(hipHostMalloc(&pinned, (hn + 2 * pg) * 4, hipHostMallocDefault));
    std::memset(pinned, 0xCD, (hn + 2 * pg) * 4);
    CK(hipHostGetDevicePointer((void**)&pinned_dev, pinned, 0));
    damage = 0;
    d = differing(x1, run_fwd(T, {dev_row(A, dP.p, carry.ptr<float>(), cfrom)}, 7, 2, &damage, {CoarseHandOver{dP.p + A.in_off, pinned_dev + pg, hn}}));
    const std::vector<float> cgot = carry.host((size_t)hl);
    size_t cbad = 0;
    for (int64_t i = 0; i < hl; i++) cbad += bits(cgot[i]) != bits(P.h[A.in_off + cfrom + i]);
    check("fwd.carry", !cbad && !d && !carry.guard_damage() && !damage, "carry differs %zu spectra differ %zu guard %zu", cbad, d, carry.guard_damage() + damage);
    size_t hbad = 0, hguard = 0;
    for (int64_t i = 0; i < hn; i++) hbad += bits(pinned[pg + i]) != bits(P.h[A.in_off + i]);
    for (size_t i = 0; i < pg; i++) hguard += !is_cd(pinned[i]) + !is_cd(pinned[pg + hn + i]);
    check("fwd.handover", !hbad && !hguard, "page-locked row differs %zu guard %zu", hbad, hguard);
    CK(hipHostFree(pinned));
  }
  // a constant 1.0 and (+1, -1, ...): a frame holds TWICE the spectrum (the 1/2 of the split is folded into the impulse responses'
  // scale), so 2 x 16384 at the first / second real of position 0 and exactly 0 everywhere else
  for (int alt = 0; alt < 2; alt++) {
    Pool P;
    RowSpec A;
    A.hist_len = 2 * CB;
    A.nvalid = 3 * CB;
    A.hist_off = (long)P.take(A.hist_len);
    A.in_off = (long)P.take(A.nvalid);
    A.u0 = 0;
    A.n_frames = 3;
    for (int64_t i = 0; i < A.hist_len; i++) P.h[A.hist_off + i] = alt && (i & 1) ? -1.f : 1.f;
    for (int64_t i = 0; i < A.nvalid; i++) P.h[A.in_off + i] = alt && (i & 1) ? -1.f : 1.f;
    DevIn<float> dP(P.h);
    size_t damage = 0, bad = 0;
    const std::vector<float> x = run_fwd(T, {dev_row(A, dP.p)}, 3, 2, &damage);
    for (int f = 0; f < 3; f++)
      for (int i = 0; i < 2 * NB; i++) bad += x[(size_t)f * 2 * NB + i] != (i == alt ? 32768.f : 0.f);
    check(alt ? "fwd.alternating" : "fwd.constant", !bad && !damage, "position 0 = (%g, %g), elements off %zu guard %zu", x[0], x[1], bad, damage);
  }
  // ---- accuracy ----
  {
    struct Shape { const char* name; bool hist, in; int64_t hist_len, nvalid; int u0, n_frames, flags; float scale; };
    const Shape shapes[] = {{"nohist", false, true, 2 * CB, 2 * CB, -1, 4, 0, 1.f},
                            {"hist1", true, true, CB, CB, -2, 4, 0, 1.f},           // u0 reaches in front of the history
                            {"hist3", true, true, 3 * CB, CB, -3, 5, 0, 1.f},
                            {"nvalid128", true, true, CB, 128, 0, 3, 0, 1.f},
                            {"nvalid_cb_minus", true, true, CB, CB - 128, 0, 3, 0, 1.f},
                            {"nvalid_cb_plus", true, true, CB, CB + 128, 0, 3, 0, 1.f},
                            {"noin", true, false, 2 * CB, 2 * CB, -1, 3, 0, 1.f},
                            {"ir", false, true, 0, 3 * CB - 640, 1, 3, 1, 1.0f / 65536.0f}};   // as Context::ensureCoarseSpectra sets it
    Pool P;
    std::vector<RowSpec> specs;
    int frames = 0;
    for (const Shape& s : shapes) {
      RowSpec r;
      if (s.hist) r.hist_off = (long)P.take(s.hist_len);
      if (s.in) r.in_off = (long)P.take(s.nvalid);
      r.nvalid = s.nvalid;
      r.hist_len = s.hist_len;
      r.u0 = s.u0;
      r.n_frames = s.n_frames;
      r.flags = s.flags;
      r.scale = s.scale;
      r.frame0 = frames;
      frames += s.n_frames;
      specs.push_back(r);
    }
    fill(P.h, 12, false);
    DevIn<float> dP(P.h);
    std::vector<CoarseXRow> rows;
    for (const RowSpec& r : specs) rows.push_back(dev_row(r, dP.p));
    size_t damage = 0;
    const std::vector<float> x = run_fwd(T, rows, frames, 2, &damage);
    struct Item { int row, f; };
    std::vector<Item> items;
    for (size_t r = 0; r < specs.size(); r++)
      for (int f = 0; f < specs[r].n_frames; f++) items.push_back(Item{(int)r, f});
    std::vector<double> rel(items.size(), 0.0), rel32(items.size(), 0.0);
    std::vector<char> wrong(items.size(), 0);
    parallel_for(items.size(), [&](size_t k) {
      const RowSpec& s = specs[items[k].row];
      const cr::XRow hr = host_row(s, P);
      const std::vector<cd> want = cr::ref_fwd_frame(hr, items[k].f);
      // the same window through a plain float32 radix-2 transform on the host (printed, not asserted)
      std::vector<double> w(cr::N);
      cr::row_window(hr, s.u0 + items[k].f, w.data());
      std::vector<float> wf(cr::N);
      for (int i = 0; i < cr::N; i++) wf[i] = (float)w[i];
      const std::vector<cf> plain = cr::spectrum_t<float>(wf.data());
      const float* g = x.data() + (size_t)(s.frame0 + items[k].f) * NB * 2;
      double e2 = 0.0, p2 = 0.0, n2 = 0.0;
      bool cdseen = false, nonzero = false;
      for (int b = 0; b < NB; b++) {
        cdseen = cdseen || is_cd(g[2 * b]) || is_cd(g[2 * b + 1]);
        nonzero = nonzero || g[2 * b] != 0.f || g[2 * b + 1] != 0.f;
        const double er = g[2 * b] - want[b].re, ei = g[2 * b + 1] - want[b].im;
        const double pr = 2.0 * plain[b].re - want[b].re, pi = 2.0 * plain[b].im - want[b].im;
        e2 += er * er + ei * ei;
        p2 += pr * pr + pi * pi;
        n2 += want[b].re * want[b].re + want[b].im * want[b].im;
      }
      if (n2 == 0.0) {
        wrong[k] = cdseen || nonzero;   // an all-zero window transforms to exact zeros
      } else {
        rel[k] = std::sqrt(e2 / n2);
        rel32[k] = std::sqrt(p2 / n2);
        wrong[k] = cdseen || !(rel[k] <= transform_bound());
      }
    });
    for (size_t r = 0; r < specs.size(); r++) {
      double worst = 0.0, worst32 = 0.0;
      int bad = 0;
      for (size_t k = 0; k < items.size(); k++)
        if (items[k].row == (int)r) {
          worst = std::max(worst, rel[k]);
          worst32 = std::max(worst32, rel32[k]);
          bad += wrong[k];
        }
      check(std::string("fwd.acc.") + shapes[r].name, !bad && !damage, "windows off %d max_rel_l2 %.3e bound %.3e ratio %.4f host_radix2_fp32 %.3e guard %zu", bad, worst,
            transform_bound(), worst / transform_bound(), worst32, damage);
    }
  }
}

static void family_inv() {
  Tables T;
  // Y rows by the reference in float64 (four signals through four two-partition responses), rounded; row 4 is zero; frame 5 of
  // every row holds values no output may read (n_y <= 5)
  const int P = 2, nT = 5, yf = 6, nrows = 5;
  Pool Pl;
  std::vector<RowSpec> xs(4), hs(4);
  for (int r = 0; r < 4; r++) {
    xs[r].hist_len = CB;
    xs[r].nvalid = (int64_t)nT * CB;
    xs[r].hist_off = (long)Pl.take(CB);
    xs[r].in_off = (long)Pl.take(xs[r].nvalid);
    xs[r].u0 = -1;
    xs[r].n_frames = nT + 1;
    hs[r].nvalid = (int64_t)P * CB;
    hs[r].in_off = (long)Pl.take(hs[r].nvalid);
    hs[r].u0 = 1;
    hs[r].n_frames = P;
    hs[r].flags = 1;
    hs[r].scale = 1.0f / 65536.0f;
  }
  const int64_t tl_max = 3 * (int64_t)CB;
  const size_t tail_off = Pl.take(tl_max);
  fill(Pl.h, 13, false);
  std::vector<float> Y((size_t)nrows * yf * NB * 2, 0.f);
  parallel_for(4, [&](size_t r) {
    const std::vector<cd> X = cr::ref_fwd(host_row(xs[r], Pl)), H = cr::ref_fwd(host_row(hs[r], Pl));
    cr::MacJob<double> J;
    J.P = P;
    J.n_t = nT;
    J.u_lo = -1;
    J.u_hi = nT - 1;
    cr::MacTerm<double> t{X.data(), 1, {}};
    t.h[0] = H.data();
    J.terms.push_back(t);
    std::vector<cd> y(NB);
    for (int tb = 0; tb < nT; tb++) {
      cr::ref_mac(J, 0, tb, y.data());
      float* dst = Y.data() + ((size_t)r * yf + tb) * NB * 2;
      for (int b = 0; b < NB; b++) {
        dst[2 * b] = (float)y[b].re;
        dst[2 * b + 1] = (float)y[b].im;
      }
    }
    float* junk = Y.data() + ((size_t)r * yf + nT) * NB * 2;
    for (int i = 0; i < 2 * NB; i++) junk[i] = 1e6f;
  });
  DevIn<float> dY(Y), dP(Pl.h);
  struct O { const char* name; std::vector<int> rows; int64_t nvalid, tail_len; bool tin, tout; int n_y; bool exact; };
  const std::vector<O> outs = {{"ny1_nvalid128", {2}, 128, 0, false, false, 5, false},
                               {"ny2_tail1", {3, 0}, CB + 384, CB, true, true, 2, false},
                               {"ny3_tail3_out_only", {1, 3, 2}, 4 * CB, 3 * CB, false, true, 5, false},   // blocks 5, 6: behind n_y
                               {"tail3_in_only", {0}, 3 * CB, 3 * CB, true, false, 3, false},
                               {"short_ny", {1, 0}, 4 * CB, CB, true, true, 2, false},                     // blocks 2 .. 4 come out as tail_in alone
                               {"no_tail", {0}, 2 * CB, 0, false, false, 5, false},
                               {"zero_y", {4}, 2 * CB + 384, 3 * CB, true, true, 3, true}};
  std::vector<int> ylist;
  std::vector<CoarseOut> co;
  std::vector<Guarded*> gout, gtail;
  int n_blocks = 0;
  for (const O& o : outs) {
    CoarseOut c{};
    gout.push_back(new Guarded((size_t)o.nvalid * 4));
    gtail.push_back(o.tout ? new Guarded((size_t)o.tail_len * 4) : nullptr);
    c.out = gout.back()->ptr<float>();
    c.nvalid = o.nvalid;
    c.y0 = (int)ylist.size();
    c.ny = (int)o.rows.size();
    for (int r : o.rows) ylist.push_back(r);
    c.tail_in = o.tin ? dP.p + tail_off : nullptr;
    c.tail_out = o.tout ? gtail.back()->ptr<float>() : nullptr;
    c.tail_len = o.tail_len;
    c.n_y = o.n_y;
    co.push_back(c);
    const int64_t send = o.nvalid + (o.tout ? o.tail_len : 0);
    n_blocks = std::max(n_blocks, (int)((send + CB - 1) / CB));
  }
  DevIn<int> dL(ylist);
  DevIn<CoarseOut> dO(co);
  const char* name = launch_coarse_inv(0, dO.p, (int)co.size(), n_blocks, dL.p, (const float2*)dY.p, yf, T.inv.p, T.ab.p);
  sync_check();
  if (std::strcmp(name, "coarse_inv_kernel")) check("inv.instance", false, "launcher returned %s", name);
  std::vector<std::string> lines(outs.size());
  std::vector<char> okv(outs.size(), 0);
  std::vector<std::vector<float>> gotO(outs.size()), gotT(outs.size());
  std::vector<size_t> dmg(outs.size(), 0);
  for (size_t k = 0; k < outs.size(); k++) {
    gotO[k] = gout[k]->host((size_t)outs[k].nvalid);
    dmg[k] = gout[k]->guard_damage();
    if (gtail[k]) {
      gotT[k] = gtail[k]->host((size_t)outs[k].tail_len);
      dmg[k] += gtail[k]->guard_damage();
    }
  }
  parallel_for(outs.size(), [&](size_t k) {
    const O& o = outs[k];
    cr::OutDesc d;
    d.nvalid = o.nvalid;
    d.rows = o.rows;
    d.tail_in = o.tin ? Pl.h.data() + tail_off : nullptr;
    d.tail_out = o.tout;
    d.tail_len = o.tail_len;
    d.n_y = o.n_y;
    const std::vector<double> v = cr::ref_inv(d, (const cf*)Y.data(), yf);
    auto got = [&](int64_t i) { return i < o.nvalid ? gotO[k][(size_t)i] : gotT[k][(size_t)(i - o.nvalid)]; };
    const int64_t send = (int64_t)v.size();
    double worst = 0.0;
    size_t bad = 0, unwritten = 0;
    for (int64_t s0 = 0; s0 < send; s0 += CB) {
      double e2 = 0.0, n2 = 0.0;
      size_t nz = 0, ne = 0;
      for (int64_t i = s0; i < std::min<int64_t>(send, s0 + CB); i++) {
        const float g = got(i);
        unwritten += is_cd(g);
        nz += g != 0.f;
        ne += bits(g) != bits((float)v[(size_t)i]) && !(g == 0.f && v[(size_t)i] == 0.0);
        e2 += (g - v[(size_t)i]) * (g - v[(size_t)i]);
        n2 += v[(size_t)i] * v[(size_t)i];
      }
      if (o.exact) bad += ne;
      else if (n2 == 0.0) bad += nz;
      else {
        const double rel = std::sqrt(e2 / n2);
        worst = std::max(worst, rel);
        bad += !(rel <= transform_bound());
      }
    }
    char buf[256];
    std::snprintf(buf, sizeof buf, "%s off %zu unwritten %zu max_rel_l2 %.3e bound %.3e ratio %.4f guard %zu", o.exact ? "elements" : "blocks", bad, unwritten, worst,
                  transform_bound(), worst / transform_bound(), dmg[k]);
    lines[k] = buf;
    okv[k] = !bad && !unwritten && !dmg[k];
  });
  for (size_t k = 0; k < outs.size(); k++) {
    check(std::string("inv.") + outs[k].name, okv[k], "%s", lines[k].c_str());
    delete gout[k];
    delete gtail[k];
  }
}

// =====================================================================================================================
//  pre-mix: out[f] = sum over the terms of in_t[f], Kahan-compensated.  Integer inputs: exact.  Uniform inputs:
//     |got - ref| <= (2 u + 8 n u^2) sum |x|,   u = 2^-24,  n = terms + 4
//  -- Kahan's bound, |error| <= (2 u + O(n u^2)) sum |x_i| (Higham, Accuracy and Stability, (4.8)); a frame's sum is made of four
//  compensated partial sums (one per wave) whose sums and corrections wave 0 adds, compensated again: at most four terms more.  The
//  header's "correctly rounded sum to within an ulp" is this bound: relative to sum |x|, not to the sum.
// =====================================================================================================================
static void family_premix() {
  const int NT[] = {0, 1, 7, 8, 9, 33, 64, 65, 257};
  // (4003 words are 63 steps: with nine summing jobs on a chip of 256 compute units wgs_per_cu = 1, 2, 4 give 28, 56 and 63
  // workgroups per job, three different grids)
  const int WORDS[] = {1, 63, 64, 65, 8 * 500 + 3};
  const int nrows = 257;
  const size_t stride = 16020;   // floats per input row: 4005 words, room for a view offset by one float
  for (int integer = 1; integer >= 0; integer--) {
    std::vector<float> pool(nrows * stride);
    fill(pool, 21 + integer, integer != 0);
    DevIn<float> dP(pool);
    for (int words : WORDS) {
      const int64_t n = 4 * (int64_t)words;
      std::vector<float> first_out;
      size_t bad = 0, cbad = 0, damage = 0, grid_diff = 0;
      double worst = 0.0;
      for (int wgs : {1, 2, 4}) {
        // arenas: every job's output and every carry between 256-byte gaps that stay 0xCD
        std::vector<PremixJob> jobs;
        std::vector<PremixTerm> terms;
        std::vector<size_t> out_off, carry_off;   // in floats
        std::vector<int64_t> cfrom;
        size_t osz = 0, csz = 0;
        std::vector<size_t> term_carry;           // per term: offset + 1, or 0
        for (int ji = 0; ji < 9; ji++) {
          const int nt = NT[ji];
          const bool aligned = (ji & 1) == 0;
          const int variant = ji % 4;             // 0: no carries; carry_from inside a 64-word step / on a step edge / = n
          int64_t cf = variant == 1 ? 4 * (64 + 17) : (variant == 2 ? 4 * 64 : n);
          cf = std::min(cf, n);
          PremixJob J{};
          J.term0 = (int)terms.size();
          J.nterms = nt;
          J.n = n;
          J.carry_from = cf;
          bool any = false;
          for (int t = 0; t < nt; t++) {
            // (job ji starts at row ji of the pool: the jobs sum different rows)
            const float* in = dP.p + (size_t)((ji + t) % nrows) * stride + (aligned ? 0 : 1);
            const bool car = variant != 0 && t % 3 == 0;
            terms.push_back(PremixTerm{in, nullptr});
            term_carry.push_back(car ? csz + 1 : 0);
            if (car) csz += (size_t)(n - cf) + 64;
            any = any || car;
          }
          J.flags = (aligned ? 1 : 0) | (any ? 2 : 0);
          out_off.push_back(osz);
          osz += (size_t)n + 64;
          cfrom.push_back(cf);
          jobs.push_back(J);
        }
        Guarded dOut(osz * 4), dCar((csz + 64) * 4);
        for (size_t j = 0; j < jobs.size(); j++) jobs[j].out = dOut.ptr<float>() + out_off[j];
        for (size_t t = 0; t < terms.size(); t++)
          if (term_carry[t]) terms[t].carry = dCar.ptr<float>() + (term_carry[t] - 1);
        DevIn<PremixJob> dJ(jobs);
        DevIn<PremixTerm> dT(terms);
        const char* name = launch_coarse_premix(0, dJ.p, (int)jobs.size(), 0, dT.p, n, wgs);
        sync_check();
        if (std::strcmp(name, "coarse_premix_kernel")) bad++;
        const std::vector<float> out = dOut.host(osz), car = dCar.host(csz + 64);
        damage += dOut.guard_damage() + dCar.guard_damage();
        std::vector<float> want_car(csz + 64, cd_float());
        std::vector<char> owritten(osz, 0);
        for (size_t j = 0; j < jobs.size(); j++) {
          std::vector<const float*> in;
          for (int t = 0; t < jobs[j].nterms; t++) {
            const float* p = pool.data() + (size_t)((j + t) % nrows) * stride + ((j & 1) == 0 ? 0 : 1);
            in.push_back(p);
            const size_t tc = term_carry[jobs[j].term0 + t];
            if (tc)
              for (int64_t f = cfrom[j]; f < n; f++) want_car[tc - 1 + (size_t)(f - cfrom[j])] = p[f];
          }
          std::vector<double> ref((size_t)n), sa((size_t)n);
          cr::ref_premix(in, n, ref.data(), sa.data());
          const double nn = jobs[j].nterms + 4;
          for (int64_t f = 0; f < n; f++) {
            const float g = out[out_off[j] + (size_t)f];
            owritten[out_off[j] + (size_t)f] = 1;
            if (is_cd(g)) { bad++; continue; }
            const double err = std::fabs((double)g - ref[(size_t)f]);
            if (integer) bad += err != 0.0;
            else {
              const double bound = (2.0 * kU + 8.0 * nn * kU * kU) * sa[(size_t)f];
              if (err != 0.0) worst = std::max(worst, err / bound);
              bad += !(err <= bound);
            }
          }
        }
        for (size_t i = 0; i < osz; i++) bad += !owritten[i] && !is_cd(out[i]);   // the gaps between the outputs
        cbad += differing(car, want_car);
        if (first_out.empty()) first_out = out;
        else grid_diff += differing(first_out, out);
      }
      const std::string tag = std::string(integer ? "int" : "uni") + ".w" + std::to_string(words);
      if (integer) check("premix." + tag, !bad && !cbad && !damage, "wrong %zu carry differs %zu guard %zu", bad, cbad, damage);
      else check("premix." + tag, !bad && !cbad && !damage, "over the bound %zu max_ratio %.4f carry differs %zu guard %zu", bad, worst, cbad, damage);
      if (!integer) check("premix.grid." + std::string("w") + std::to_string(words), !grid_diff, "wgs_per_cu 1 against 2, 4: differ %zu", grid_diff);
    }
    if (integer) continue;
    // one hand-over job (a plain copy to page-locked host memory) in front of two summing jobs
    const int64_t n = 3212, hn = n;   // 803 words
    float* pinned = nullptr;
    float* pinned_dev = nullptr;
    const size_t pg = 1024;
    CK(hipHostMalloc(&pinned, (hn + 2 * pg) * 4, hipHostMallocDefault));
    std::memset(pinned, 0xCD, (hn + 2 * pg) * 4);
    CK(hipHostGetDevicePointer((void**)&pinned_dev, pinned, 0));
    Guarded dOut((size_t)(2 * n + 64) * 4);
    std::vector<PremixTerm> terms = {PremixTerm{dP.p + 5 * stride, nullptr}};
    std::vector<PremixJob> jobs(3);
    jobs[0] = PremixJob{pinned_dev + pg, 0, 1, hn, hn, 1 | 4, 0};
    for (int j = 0; j < 2; j++) {
      jobs[1 + j] = PremixJob{dOut.ptr<float>() + (size_t)j * (n + 64), (int)terms.size(), 9 + 8 * j, n, n, 1, 0};
      for (int t = 0; t < 9 + 8 * j; t++) terms.push_back(PremixTerm{dP.p + (size_t)(10 * j + t) * stride, nullptr});
    }
    DevIn<PremixJob> dJ(jobs);
    DevIn<PremixTerm> dT(terms);
    launch_coarse_premix(0, dJ.p, 3, 1, dT.p, n, 2);
    sync_check();
    size_t hbad = 0, hguard = 0, sbad = 0;
    for (int64_t i = 0; i < hn; i++) hbad += bits(pinned[pg + i]) != bits(pool[5 * stride + i]);
    for (size_t i = 0; i < pg; i++) hguard += !is_cd(pinned[i]) + !is_cd(pinned[pg + hn + i]);
    const std::vector<float> out = dOut.host((size_t)(2 * n + 64));
    for (int j = 0; j < 2; j++) {
      std::vector<const float*> in;
      for (int t = 0; t < 9 + 8 * j; t++) in.push_back(pool.data() + (size_t)(10 * j + t) * stride);
      std::vector<double> ref((size_t)n), sa((size_t)n);
      cr::ref_premix(in, n, ref.data(), sa.data());
      for (int64_t f = 0; f < n; f++) {
        const float g = out[(size_t)j * (n + 64) + f];
        sbad += is_cd(g) || !(std::fabs((double)g - ref[(size_t)f]) <= (2.0 * kU + 8.0 * (13 + 8 * j) * kU * kU) * sa[(size_t)f]);
      }
    }
    for (int i = 0; i < 64; i++) sbad += !is_cd(out[(size_t)n + i]);
    check("premix.handover", !hbad && !hguard && !sbad && !dOut.guard_damage(), "page-locked row differs %zu guard %zu sums off %zu device guard %zu", hbad, hguard, sbad,
          dOut.guard_damage());
    CK(hipHostFree(pinned));
  }
}

// =====================================================================================================================
//  history: the last hist_len samples of [old history | this chunk's input], exact
// =====================================================================================================================
static void family_hist() {
  const int64_t hl = 2 * CB;
  struct Case { const char* name; bool old, in; int64_t n; int mis; };
  const Case cases[] = {{"old_null", false, true, 128 * 5, 0}, {"in_null", true, false, 128 * 5, 0},    {"n_below", true, true, 128 * 5, 0},
                        {"n_equal", true, true, hl, 0},        {"n_above", true, true, hl + CB + 128, 0}, {"unaligned_in", true, true, 128 * 7, 1}};
  Pool P;
  std::vector<size_t> oo, io;
  for (const Case& c : cases) {
    oo.push_back(P.take(hl));
    io.push_back(P.take(c.n, c.mis));
  }
  fill(P.h, 31, false);
  DevIn<float> dP(P.h);
  std::vector<Guarded*> g;
  std::vector<CoarseHistJob> jobs;
  for (size_t k = 0; k < 6; k++) {
    g.push_back(new Guarded((size_t)hl * 4));
    jobs.push_back(CoarseHistJob{cases[k].old ? dP.p + oo[k] : nullptr, cases[k].in ? dP.p + io[k] : nullptr, g[k]->ptr<float>(), hl, cases[k].n});
  }
  DevIn<CoarseHistJob> dJ(jobs);
  launch_coarse_hist(0, dJ.p, (int)jobs.size(), hl);
  sync_check();
  for (size_t k = 0; k < 6; k++) {
    const std::vector<float> want = cr::ref_hist(cases[k].old ? P.h.data() + oo[k] : nullptr, cases[k].in ? P.h.data() + io[k] : nullptr, hl, cases[k].n);
    const size_t d = differing(g[k]->host((size_t)hl), want), dm = g[k]->guard_damage();
    check(std::string("hist.") + cases[k].name, !d && !dm, "differ %zu guard %zu", d, dm);
    delete g[k];
  }
}

// =====================================================================================================================
//  one convolution end to end on the device: forward on the taps and on the signal, multiply-accumulate, inverse, against direct
//  float64 convolution.  The bound is the render tests' own (tests/test_gpu_coarse.py, REL = 2e-6), here on the largest error against
//  the output's peak; the rms ratio is printed next to it.
// =====================================================================================================================
static void family_chain() {
  Tables T;
  const int64_t taps = 20000, stride = 20096;   // (whole 128-frame blocks, as the engine stores the taps)
  const int P = (int)((stride + CB - 1) / CB), nT = 5;
  const int64_t n = (int64_t)nT * CB - 384, hl = (int64_t)P * CB;
  Pool Pl;
  RowSpec h, x;
  h.in_off = (long)Pl.take(stride);
  h.nvalid = stride;
  h.u0 = 1;
  h.n_frames = P;
  h.flags = 1;
  h.scale = 1.0f / 65536.0f;
  h.frame0 = 0;
  x.hist_off = (long)Pl.take(hl);
  x.in_off = (long)Pl.take(n);
  x.hist_len = hl;
  x.nvalid = n;
  x.u0 = -(P - 1);
  x.n_frames = nT + P - 1;
  x.frame0 = P;
  fill(Pl.h, 41, false);
  for (int64_t i = taps; i < stride; i++) Pl.h[h.in_off + i] = 0.f;
  DevIn<float> dP(Pl.h);
  const int frames = P + x.n_frames;
  Guarded dX((size_t)frames * NB * 8), dY((size_t)nT * NB * 8), dO((size_t)n * 4);
  {
    DevIn<CoarseXRow> dH(std::vector<CoarseXRow>{dev_row(h, dP.p)});
    launch_coarse_fwd(0, dH.p, 1, P, P, dX.ptr<float2>(), T.fwd.p, T.ab.p);
    DevIn<CoarseXRow> dR(std::vector<CoarseXRow>{dev_row(x, dP.p)});
    launch_coarse_fwd(0, dR.p, 1, x.n_frames, 2, dX.ptr<float2>(), T.fwd.p, T.ab.p);
    sync_check();
  }
  CoarseTerm t{};
  t.frame0 = x.frame0 - x.u0 - (P - 1);
  t.h[0] = dX.ptr<float2>();
  CoarseJob J{};
  J.n_terms = 1;
  J.P = P;
  J.n_t = nT;
  J.u_lo = -(P - 1);
  J.u_hi = nT - 1;
  DevIn<CoarseTerm> dT(std::vector<CoarseTerm>{t});
  DevIn<CoarseJob> dJ(std::vector<CoarseJob>{J});
  launch_coarse_mac(0, dJ.p, 1, dT.p, dX.ptr<float2>(), dY.ptr<float2>(), nT, 1, nT, P, true, 1, false);
  CoarseOut o{};
  o.out = dO.ptr<float>();
  o.nvalid = n;
  o.ny = 1;
  o.n_y = nT;
  DevIn<CoarseOut> dOut(std::vector<CoarseOut>{o});
  DevIn<int> dL(std::vector<int>{0});
  launch_coarse_inv(0, dOut.p, 1, nT, dL.p, dY.ptr<float2>(), nT, T.inv.p, T.ab.p);
  sync_check();
  const std::vector<float> got = dO.host((size_t)n);
  std::vector<double> s((size_t)(hl + n)), hd((size_t)taps), want((size_t)n);
  for (int64_t i = 0; i < hl; i++) s[(size_t)i] = Pl.h[x.hist_off + i];
  for (int64_t i = 0; i < n; i++) s[(size_t)(hl + i)] = Pl.h[x.in_off + i];
  for (int64_t k = 0; k < taps; k++) hd[(size_t)k] = Pl.h[h.in_off + k];
  parallel_for((size_t)((n + 255) / 256), [&](size_t blk) {
    for (int64_t i = (int64_t)blk * 256; i < std::min<int64_t>(n, (int64_t)(blk + 1) * 256); i++) {
      double acc = 0.0;
      const double* si = s.data() + hl + i;
      for (int64_t k = 0; k < taps; k++) acc += hd[(size_t)k] * si[-k];
      want[(size_t)i] = acc;
    }
  });
  double peak = 0.0, worst = 0.0, e2 = 0.0, n2 = 0.0;
  size_t unwritten = 0;
  for (int64_t i = 0; i < n; i++) {
    unwritten += is_cd(got[(size_t)i]);
    peak = std::max(peak, std::fabs(want[(size_t)i]));
    worst = std::max(worst, std::fabs(got[(size_t)i] - want[(size_t)i]));
    e2 += (got[(size_t)i] - want[(size_t)i]) * (got[(size_t)i] - want[(size_t)i]);
    n2 += want[(size_t)i] * want[(size_t)i];
  }
  const size_t dm = dX.guard_damage() + dY.guard_damage() + dO.guard_damage();
  check("chain.convolution", !unwritten && !dm && worst <= 2e-6 * peak, "max_err/peak %.3e bound 2e-6 ratio %.4f rms_err/rms %.3e unwritten %zu guard %zu", worst / peak,
        worst / peak / 2e-6, std::sqrt(e2 / n2), unwritten, dm);
}

int main(int argc, char** argv) {
  const std::string fam = argc > 1 ? argv[1] : "";
  const auto t0 = std::chrono::steady_clock::now();
  gDry = argc > 2 && std::string(argv[2]) == "dry" && (fam == "mac" || fam == "mac_float");
  if (fam == "mac") family_mac();
  else if (fam == "mac_float") family_mac_float();
  else if (fam == "fwd") family_fwd();
  else if (fam == "inv") family_inv();
  else if (fam == "premix") family_premix();
  else if (fam == "hist") family_hist();
  else if (fam == "chain") family_chain();
  else {
    std::printf("usage: coarse_kernels_check mac|mac_float|fwd|inv|premix|hist|chain\n");
    return 2;
  }
  std::printf("family %s: %d checks failed, %.2f s\n", fam.c_str(), failures, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  return failures ? 1 : 0;
}
