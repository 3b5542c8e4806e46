// Stand-alone run of the time-split biquad path of graphaudio_amd/csrc/ga_biquad.hip through its launchers alone, on plain device tables,
// against tests/biquad_split_ref.hpp.  argv[1] picks a family:
//   scan    launch_biquad_scan alone on integers: biquad_scan_fixed_kernel<1..4> (nsec = k) and biquad_scan_kernel (nsec = 0, and k >= 5)
//   expand  launch_biquad_split_expand: the passA / passB job tables field by field
//   pipe    expand -> launch_biquad_lanes(state_only) -> launch_biquad_scan -> launch_biquad_lanes, in the order of
//           ga_chunk_internal.hpp (Exec::flushLevel), two segments in a row: outputs, scratch and persistent states bit for bit
// The path is fully determined: both passes are the float32 recurrence of BiQuadFilterNode.cs:137-138 operation by operation, the scan
// is float64 in a stated order with two stated float roundings, and the library is built with -ffp-contract=off -- so every comparison
// here is ==, on bits.
// scan: s_0, z_l and A^K are small integers, A^K non-symmetric and different per job, stored at offsets that are not in job order; for
// G = 256 it is a signed cyclic permutation so that values stay bounded.  The host model asserts that every value stays below 2^24.
// Outputs, scratch, states and job tables lie between guard regions filled with the byte 0xCD like the arrays themselves: the guards
// must be untouched afterwards, and every element the contract says is not written must still read 0xCD.  Inputs (samples, A^K,
// sections, cascades) lie between guard regions of NaN, and every input sample the contract says is not read is NaN.
// Each check prints one line, "check <name> ok|FAIL <figures>"; the program exits with status 1 if any check fails, and at once with
// status 3 after a HIP error (the caller then starts nothing more).  (tests/test_gpu_biquad_split_kernels.py holds the check names.)
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "ga_kernels.hpp"
#include "biquad_split_ref.hpp"

using namespace ga;
namespace br = bq_ref;
static_assert(sizeof(BiquadJob) == 56 && sizeof(BiquadScanJob) == 64 && sizeof(BiquadSection) == 32, "records without padding: compared as bytes");

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
  std::printf("check %s %s %s\n", name.c_str(), ok ? "ok" : "FAIL", buf);
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
  double unit() { return ((double)(next() >> 11) + 0.5) / 9007199254740992.0; }   // (0, 1)
  float gauss() { return (float)(std::sqrt(-2.0 * std::log(unit())) * std::cos(6.283185307179586 * unit())); }
  int small_int(int m) { return (int)(next() % (uint64_t)(2 * m + 1)) - m; }   // [-m, m]
};

template <class F>
static void parallel_for(size_t n, F f) {   // the host model: at most 16 threads
  const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::atomic<size_t> next{0};
  std::vector<std::thread> th;
  for (unsigned i = 0; i < nt; i++)
    th.emplace_back([&] {
      for (size_t k; (k = next.fetch_add(1)) < n;) f(k);
    });
  for (auto& t : th) t.join();
}

constexpr uint32_t kCD = 0xCDCDCDCDu, kNaN = 0x7FC00000u;   // (two kNaN words are a float64 NaN as well)
static float from_bits(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
static int64_t roundup(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// device array of exactly `bytes` (a multiple of 4) between two guard regions; array and guards start as the 32-bit word `word`
struct Guarded {
  char* raw = nullptr;
  size_t bytes, g;
  uint32_t word;
  explicit Guarded(size_t bytes_, uint32_t word_ = kCD, size_t guard = 65536) : bytes(bytes_), g(guard), word(word_) {
    CK(hipMalloc(&raw, g + bytes + g + 4));
    CK(hipMemsetD32((hipDeviceptr_t)raw, (int)word, (g + bytes + g) / 4));
  }
  ~Guarded() { (void)hipFree(raw); }
  Guarded(const Guarded&) = delete;
  Guarded& operator=(const Guarded&) = delete;
  template <class T>
  T* ptr(size_t byte_off = 0) const { return (T*)(raw + g + byte_off); }
  void upload(const void* src, size_t n, size_t byte_off = 0) { CK(hipMemcpy(raw + g + byte_off, src, n, hipMemcpyHostToDevice)); }
  void refill() { CK(hipMemsetD32((hipDeviceptr_t)(raw + g), (int)word, bytes / 4)); }
  void zero() { CK(hipMemset(raw + g, 0, bytes)); }
  template <class T>
  std::vector<T> host() const {
    std::vector<T> h(bytes / sizeof(T));
    CK(hipDeviceSynchronize());
    if (bytes) CK(hipMemcpy(h.data(), raw + g, bytes, hipMemcpyDeviceToHost));
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
static void sync() {
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
}
template <class T>
static size_t differing(const std::vector<T>& a, const std::vector<T>& b, long long* first = nullptr) {   // on bits
  size_t bad = a.size() == b.size() ? 0 : 1;
  for (size_t i = 0; i < a.size() && i < b.size(); i++)
    if (std::memcmp(&a[i], &b[i], sizeof(T)) != 0) {
      if (!bad && first) *first = (long long)i;
      bad++;
    }
  return bad;
}
static int perm(int j, int n) { return (int)(((int64_t)17 * j + 3) % n); }   // (17 is coprime to every count used here)

// ================================================================ scan ================================================================
static void scan_case(int k, int G, int njobs) {
  const int D = 2 * k;
  const std::string name = fmt("scan.s%d.G%d.n%d", k, G, njobs);
  Rng rng{0x5CA0000ull + (uint64_t)k * 1000003 + (uint64_t)G * 131 + (uint64_t)njobs};
  // A^K per job: G <= 5: three entries of +-1 per row (D = 2: entries in [-2, 2]); G = 256: a signed cyclic shift.  Never symmetric.
  std::vector<std::vector<double>> M(njobs, std::vector<double>((size_t)D * D));
  for (int j = 0; j < njobs; j++) {
    for (bool sym = true; sym;) {
      std::fill(M[j].begin(), M[j].end(), 0.0);
      for (int r = 0; r < D; r++) {
        if (G > 5) M[j][(size_t)r * D + (r + 1 + j % (D - 1 > 0 ? D - 1 : 1)) % D] = (rng.next() & 1) ? 1.0 : -1.0;
        else if (D == 2) { M[j][r * 2] = rng.small_int(2); M[j][r * 2 + 1] = rng.small_int(2); }
        else for (int e = 0; e < 3; e++) M[j][(size_t)r * D + (int)(rng.next() % D)] = (rng.next() & 1) ? 1.0 : -1.0;
      }
      sym = true;
      for (int r = 0; r < D; r++)
        for (int c = 0; c < D; c++) sym = sym && M[j][(size_t)r * D + c] == M[j][(size_t)c * D + r];
    }
  }
  // tables: 16 bytes of padding, then job j's matrix in slot perm(j)
  const size_t mbytes = (size_t)D * D * 8;
  std::vector<uint8_t> blob(16 + mbytes * njobs);
  {
    const uint32_t nanw = kNaN;
    for (size_t i = 0; i < blob.size(); i += 4) std::memcpy(&blob[i], &nanw, 4);
  }
  std::vector<BiquadScanJob> jobs(njobs);
  std::vector<BiquadSection> secs(1 + (size_t)njobs * k);
  const size_t nscratch = (size_t)njobs * (G - 1) * D, nstate = (size_t)njobs * D;
  Guarded d_blob(blob.size(), kNaN), d_jobs(jobs.size() * sizeof(BiquadScanJob), kNaN), d_secs(secs.size() * sizeof(BiquadSection), kNaN);
  Guarded d_scratch(nscratch * 4), d_state(nstate * 4);
  std::vector<float> scratch0(nscratch), state0(nstate);
  for (auto& v : scratch0) v = (float)rng.small_int(7);
  for (auto& v : state0) v = (float)rng.small_int(7);
  std::memset(&secs[0], 0, sizeof(BiquadSection));   // (a section nobody owns: sec0 is never 0)
  for (int j = 0; j < njobs; j++) {
    const int slot = perm(j, njobs), srow = perm(njobs - 1 - j, njobs);   // matrices, scratch and sections each in another order
    std::memcpy(&blob[16 + mbytes * slot], M[j].data(), mbytes);
    BiquadScanJob& J = jobs[j];
    J.in = nullptr;
    J.out = nullptr;
    J.m_off = 16 + mbytes * slot;
    J.scratch = d_scratch.ptr<float>() + (size_t)srow * (G - 1) * D;
    J.sec0 = 1 + slot * k;
    J.nsec = k;
    J.f0 = 0;
    J.n = 0;
    J.twins = 1;
    J.pad_ = 0;
    for (int q = 0; q < k; q++) {
      BiquadSection& s = secs[(size_t)J.sec0 + q];
      s.b0 = s.b1 = s.b2 = s.a1 = s.a2 = s.pad_ = 0.f;
      s.state = d_state.ptr<float>() + (size_t)slot * D + 2 * q;
    }
  }
  // the model, job by job, in the arrays' own layout; every value below 2^24
  std::vector<float> scratch_exp = scratch0, state_exp = state0;
  double biggest = 0;
  for (int j = 0; j < njobs; j++) {
    const int slot = perm(j, njobs), srow = perm(njobs - 1 - j, njobs);
    br::scan(M[j].data(), D, G, scratch_exp.data() + (size_t)srow * (G - 1) * D, state_exp.data() + (size_t)slot * D);
  }
  for (float v : scratch_exp) biggest = std::max(biggest, (double)std::fabs(v));
  for (float v : state_exp) biggest = std::max(biggest, (double)std::fabs(v));
  // (|s_{l+1}| <= 3 |s_l| + 7 for G <= 5, <= |s_l| + 7 for the shifts: every partial sum is bounded by the next state's bound)
  const double growth = G > 5 ? 7.0 * G : 7.0 * std::pow(D == 2 ? 4.0 : 3.0, G) * 2;
  if (growth >= 16777216.0 || biggest >= 16777216.0) {
    check(name, false, "the integer model leaves 2^24: bound %g, largest %g", growth, biggest);
    return;
  }
  d_blob.upload(blob.data(), blob.size());
  d_jobs.upload(jobs.data(), jobs.size() * sizeof(BiquadScanJob));
  d_secs.upload(secs.data(), secs.size() * sizeof(BiquadSection));
  std::vector<float> got_scratch[2], got_state[2];
  for (int pass = 0; pass < 2; pass++) {   // nsec = k: the fixed kernels for k <= 4 ; nsec = 0: the generic kernel for every k
    if (nscratch) d_scratch.upload(scratch0.data(), nscratch * 4);
    d_state.upload(state0.data(), nstate * 4);
    launch_biquad_scan(0, d_jobs.ptr<BiquadScanJob>(), njobs, G, d_secs.ptr<BiquadSection>(), d_blob.ptr<uint8_t>(), pass == 0 ? k : 0);
    sync();
    got_scratch[pass] = d_scratch.host<float>();
    got_state[pass] = d_state.host<float>();
  }
  long long first = -1;
  const size_t b0 = differing(got_scratch[0], scratch_exp, &first), b1 = differing(got_scratch[1], scratch_exp, &first);
  const size_t c0 = differing(got_state[0], state_exp), c1 = differing(got_state[1], state_exp);
  const size_t eq = differing(got_scratch[0], got_scratch[1]) + differing(got_state[0], got_state[1]);
  const size_t dmg = d_scratch.guard_damage() + d_state.guard_damage() + d_blob.guard_damage() + d_jobs.guard_damage() + d_secs.guard_damage();
  check(name, b0 + b1 + c0 + c1 + eq + dmg == 0, "scratch differing %zu / %zu of %zu (first %lld), state %zu / %zu of %zu, nsec=k vs nsec=0 %zu, guard words %zu, largest |value| %g",
        b0, b1, nscratch, first, c0, c1, nstate, eq, dmg, biggest);
}
static void family_scan() {
  for (int k = 1; k <= 8; k++)
    for (int G : {1, 2, 3, 5, 256})
      for (int njobs : {1, 64, 65, 130}) scan_case(k, G, njobs);
}

// =============================================================== expand ===============================================================
static void expand_case(int ncasc, int G, int64_t K, int64_t last, int twins) {
  const std::string name = fmt("expand.c%dxG%d.K%lld.last%lld.t%d", ncasc, G, (long long)K, (long long)last, twins);
  Guarded d_casc((size_t)ncasc * sizeof(BiquadScanJob), kNaN), d_pa((size_t)ncasc * (G - 1) * sizeof(BiquadJob)), d_pb((size_t)ncasc * G * sizeof(BiquadJob));
  // (the views and the scratch are never touched by this kernel: any distinct addresses do)
  float* const fake = (float*)(uintptr_t)0x100000000ull;
  std::vector<BiquadScanJob> casc(ncasc);
  std::vector<BiquadJob> pa_exp, pb_exp;
  for (int j = 0; j < ncasc; j++) {
    BiquadScanJob& C = casc[j];
    C.nsec = 1 + j % 8;
    C.in = fake + (size_t)j * 1000003;
    C.out = fake + (size_t)j * 1000003 + 500000000ull;
    C.m_off = 16 + 64 * (uint64_t)j;
    C.scratch = fake + 2000000000ull + (size_t)j * 4096;
    C.sec0 = 3 * j + 1;
    C.f0 = 128 * (j % 5);
    C.n = (G - 1) * K + last;
    C.twins = twins;
    C.pad_ = 0;
    std::vector<br::Piece> pa, pb;
    br::expand(C.f0, C.n, C.nsec, C.twins, G, K, pa, pb);
    auto job = [&](const br::Piece& p) {
      BiquadJob b;
      b.in = C.in;
      b.out = p.out ? C.out : nullptr;
      b.sec0 = C.sec0;
      b.nsec = C.nsec;
      b.f0 = p.f0;
      b.n = p.n;
      b.state = p.state_off >= 0 ? C.scratch + p.state_off : nullptr;
      b.twins = p.twins;
      b.pad_ = 0;
      return b;
    };
    for (const br::Piece& p : pa) pa_exp.push_back(job(p));
    for (const br::Piece& p : pb) pb_exp.push_back(job(p));
  }
  d_casc.upload(casc.data(), casc.size() * sizeof(BiquadScanJob));
  launch_biquad_split_expand(0, d_casc.ptr<BiquadScanJob>(), ncasc, G, K, d_pa.ptr<BiquadJob>(), d_pb.ptr<BiquadJob>());
  sync();
  const std::vector<BiquadJob> pa = d_pa.host<BiquadJob>(), pb = d_pb.host<BiquadJob>();
  long long fa = -1, fb = -1;
  const size_t ba = differing(pa, pa_exp, &fa), bb = differing(pb, pb_exp, &fb);
  const size_t dmg = d_pa.guard_damage() + d_pb.guard_damage() + d_casc.guard_damage();
  check(name, ba + bb + dmg == 0 && pa_exp.size() == (size_t)ncasc * (G - 1) && pb_exp.size() == (size_t)ncasc * G,
        "passA records differing %zu of %zu (first %lld), passB %zu of %zu (first %lld), guard words %zu", ba, pa_exp.size(), fa, bb, pb_exp.size(), fb, dmg);
}
static void family_expand() {
  const int shapes[][2] = {{1, 2}, {3, 3}, {1, 256}, {128, 2}, {43, 6}};   // 128 x 2 = 256 threads, 43 x 6 = 258
  for (auto& s : shapes)
    for (int twins : {1, 2}) {
      expand_case(s[0], s[1], 32, 32, twins);
      expand_case(s[0], s[1], 1024, 1024, twins);
      expand_case(s[0], s[1], 1024, 32, twins);
    }
}

// ================================================================ pipe ================================================================
struct Filter { br::Type t; double f, q, g; };
static const Filter kLow[] = {
    {br::kLowpass, 40.0, 0.707, 0.0}, {br::kLowpass, 200.0, 10.0, 0.0}, {br::kHighpass, 30.0, 0.707, 0.0},  {br::kHighpass, 80.0, 10.0, 0.0}, {br::kBandpass, 60.0, 8.0, 0.0},
    {br::kNotch, 50.0, 10.0, 0.0},    {br::kPeaking, 100.0, 10.0, 12.0}, {br::kLowshelf, 60.0, 1.0, -12.0}, {br::kAllpass, 300.0, 5.0, 0.0},
};
static const Filter kMid[] = {
    {br::kPeaking, 1500.0, 1.0, 5.0}, {br::kPeaking, 5000.0, 1.0, 5.0}, {br::kLowpass, 3000.0, 0.707, 0.0}, {br::kHighpass, 2000.0, 1.0, 0.0},
    {br::kBandpass, 4000.0, 2.0, 0.0}, {br::kNotch, 7000.0, 1.5, 0.0},  {br::kLowshelf, 2500.0, 0.8, 4.0},  {br::kHighshelf, 12000.0, 1.0, 9.0}, {br::kAllpass, 9000.0, 0.9, 0.0},
};
struct PipeCase {
  std::string name;
  int k;
  bool low;       // low cut-offs (max |A^K| >= 1 is asserted) or mid-band sections
  int64_t K;
  int G;
  int64_t last;   // frames of the last piece of both segments
  int ncasc, twins;
  bool silent;    // the input falls silent after a quarter of the first segment
};
static void pipe_case(const PipeCase& pc) {
  const int k = pc.k, D = 2 * k, G = pc.G, G2 = 2, ncasc = pc.ncasc, twins = pc.twins;
  const int64_t K = pc.K, n1 = (G - 1) * K + pc.last, n2 = (G2 - 1) * K + pc.last;
  // a view: [0, 128) never touched | segment 1 | never touched up to the next multiple of 32 and 32 more | segment 2 | 32 or more never touched
  const int64_t f0a = 128, f0b = f0a + roundup(n1, 32) + 32, stride = f0b + roundup(n2, 32) + 32;
  uint64_t seed = 1469598103934665603ull;   // FNV-1a of the case's name
  for (char c : pc.name) seed = (seed ^ (uint8_t)c) * 1099511628211ull;
  Rng rng{seed};
  const int nsets = std::min(ncasc, 5);
  std::vector<std::vector<br::Sec>> sets(nsets);
  std::vector<std::vector<double>> Ms(nsets);
  double maxM = 0;
  for (int i = 0; i < nsets; i++) {
    for (int q = 0; q < k; q++) {
      const Filter& f = pc.low ? kLow[(i + 2 * q + k) % 9] : kMid[(i + 2 * q + k) % 9];
      sets[i].push_back(br::rbj(f.t, f.f * (1.0 + 0.03 * i), f.q, f.g));
    }
    const std::vector<long double> A = br::transition_seq(sets[i].data(), k, K);
    for (long double v : A) {
      Ms[i].push_back((double)v);
      maxM = std::max(maxM, std::fabs((double)v));
    }
  }
  if (pc.low && maxM < 1.0) {   // (a case must not decay into the one where the scan multiplies by nothing)
    check(pc.name, false, "max |A^K| %g < 1: the case does not carry state across a piece", maxM);
    return;
  }
  // host arrays
  const size_t nview = (size_t)ncasc * stride, nstate = (size_t)ncasc * k * twins * 2, nscr = (size_t)ncasc * (G - 1) * D;
  std::vector<float> x(nview, from_bits(kNaN)), state0(nstate, from_bits(kCD));
  for (int j = 0; j < ncasc; j++) {
    float* v = x.data() + (size_t)j * stride;
    for (int64_t i = 0; i < n1; i++) v[f0a + i] = (pc.silent && i >= n1 / 4) ? 0.f : rng.gauss();
    for (int64_t i = 0; i < n2; i++) v[f0b + i] = pc.silent ? 0.f : rng.gauss();
    for (int q = 0; q < k; q++) {   // s_0 in twin 0's slot; the other twins' slots are only ever written
      state0[((size_t)j * k + q) * twins * 2] = 0.5f * rng.gauss();
      state0[((size_t)j * k + q) * twins * 2 + 1] = 0.5f * rng.gauss();
    }
  }
  const size_t mbytes = (size_t)D * D * 8;
  std::vector<uint8_t> blob(16 + mbytes * ncasc);
  {
    const uint32_t nanw = kNaN;
    for (size_t i = 0; i < 16; i += 4) std::memcpy(&blob[i], &nanw, 4);
  }
  Guarded d_in(nview * 4, kNaN), d_out(nview * 4), d_state(nstate * 4), d_scr(nscr * 4), d_blob(blob.size(), kNaN);
  Guarded d_secs((size_t)ncasc * k * sizeof(BiquadSection), kNaN), d_casc((size_t)ncasc * sizeof(BiquadScanJob), kNaN);
  Guarded d_pa((size_t)ncasc * (G - 1) * sizeof(BiquadJob)), d_pb((size_t)ncasc * G * sizeof(BiquadJob));
  std::vector<BiquadSection> secs((size_t)ncasc * k);
  std::vector<BiquadScanJob> casc(ncasc);
  for (int j = 0; j < ncasc; j++) {
    const int slot = perm(j, ncasc);
    std::memcpy(&blob[16 + mbytes * slot], Ms[j % nsets].data(), mbytes);
    for (int q = 0; q < k; q++) {
      const br::Sec& s = sets[j % nsets][q];
      BiquadSection& o = secs[(size_t)j * k + q];
      o.b0 = s.b0; o.b1 = s.b1; o.b2 = s.b2; o.a1 = s.a1; o.a2 = s.a2;
      o.pad_ = 0.f;
      o.state = d_state.ptr<float>() + ((size_t)j * k + q) * twins * 2;
    }
    BiquadScanJob& C = casc[j];
    C.in = d_in.ptr<float>() + (size_t)j * stride;
    C.out = d_out.ptr<float>() + (size_t)j * stride;
    C.m_off = 16 + mbytes * slot;
    C.scratch = d_scr.ptr<float>() + (size_t)j * (G - 1) * D;
    C.sec0 = j * k;
    C.nsec = k;
    C.twins = twins;
    C.pad_ = 0;
  }
  d_in.upload(x.data(), nview * 4);
  d_state.upload(state0.data(), nstate * 4);
  d_blob.upload(blob.data(), blob.size());
  d_secs.upload(secs.data(), secs.size() * sizeof(BiquadSection));
  // the model's arrays, in the device layout
  std::vector<float> y(nview, from_bits(kCD)), state = state0, scr(nscr, 0.f);
  size_t bad_out = 0, bad_scr = 0, bad_state = 0, nan_out = 0;
  long long first = -1;
  for (int seg = 0; seg < 2; seg++) {
    const int g = seg == 0 ? G : G2;
    const int64_t f0 = seg == 0 ? f0a : f0b, n = seg == 0 ? n1 : n2;
    std::fill(scr.begin(), scr.end(), 0.f);
    parallel_for((size_t)ncasc, [&](size_t j) {
      br::split_f32(sets[j % nsets].data(), k, Ms[j % nsets].data(), x.data() + j * stride + f0, y.data() + j * stride + f0, n, g, K, twins,
                    state.data() + j * k * twins * 2, scr.data() + j * (G - 1) * D);
    });
    for (auto& C : casc) {
      C.f0 = f0;
      C.n = n;
    }
    d_casc.upload(casc.data(), casc.size() * sizeof(BiquadScanJob));
    d_scr.zero();   // (the planner's blocks are zeroed before pass A)
    d_pa.refill();
    d_pb.refill();
    const BiquadScanJob* cd = d_casc.ptr<BiquadScanJob>();
    const BiquadSection* sd = d_secs.ptr<BiquadSection>();
    launch_biquad_split_expand(0, cd, ncasc, g, K, d_pa.ptr<BiquadJob>(), d_pb.ptr<BiquadJob>());
    launch_biquad_lanes(0, d_pa.ptr<BiquadJob>(), ncasc * (g - 1), sd, k, true);
    launch_biquad_scan(0, cd, ncasc, g, sd, d_blob.ptr<uint8_t>(), k);
    launch_biquad_lanes(0, d_pb.ptr<BiquadJob>(), ncasc * g, sd, k);
    sync();
    const std::vector<float> go = d_out.host<float>(), gs = d_scr.host<float>(), gst = d_state.host<float>();
    bad_out += differing(go, y, &first);
    bad_scr += differing(gs, scr);
    bad_state += differing(gst, state);
    for (float v : go) nan_out += std::isnan(v);
  }
  const size_t dmg = d_in.guard_damage() + d_out.guard_damage() + d_state.guard_damage() + d_scr.guard_damage() + d_blob.guard_damage() +
                     d_secs.guard_damage() + d_casc.guard_damage() + d_pa.guard_damage() + d_pb.guard_damage();
  size_t subnormal = 0;   // (in the model's outputs: the silent case has to pass through them)
  for (float v : y) subnormal += v != 0.f && std::fabs(v) < 1.17549435e-38f;
  const bool ok = bad_out + bad_scr + bad_state + nan_out + dmg == 0 && (!pc.silent || subnormal > 0);
  check(pc.name, ok, "outputs differing %zu of %zu (first %lld), scratch %zu of %zu, states %zu of %zu, NaN in outputs %zu, guard words %zu; max |A^K| %.3g, "
        "subnormal outputs %zu", bad_out, 2 * nview, first, bad_scr, 2 * nscr, bad_state, 2 * nstate, nan_out, dmg, maxM, subnormal);
}
static void family_pipe() {
  std::vector<PipeCase> cases;
  auto add = [&](const char* tag, int k, bool low, int64_t K, int G, int64_t last, int ncasc, int twins, bool silent = false) {
    cases.push_back(PipeCase{fmt("pipe.%ss%d.%s.K%lld.G%d.c%d.t%d%s", tag, k, low ? "low" : "mid", (long long)K, G, ncasc, twins, silent ? ".silent" : ""),
                             k, low, K, G, last, ncasc, twins, silent});
  };
  for (int k = 1; k <= 8; k++) {
    add("", k, true, 32, 7, 32, 65, 1);       // biquad1_kernel's one round
    add("", k, true, 64, 3, 64, 33, 2);       // the `more` prefetch and its end
    add("", k, true, 96, 2, 32, 1, 3);        // ... and a last piece shorter than the others
    add("", k, true, 1056, 3, 1056, 33, 1);   // many tiles
    add("", k, false, 1056, 7, 64, 1, 2);     // one mid-band cascade per length
  }
  add("", 3, false, 1056, 3, 1056, 1, 1, true);   // the states decay through the subnormals
  add("", 2, true, 32, 256, 32, 70, 1);           // 70 x 255 = 17,850 pass-A jobs: launch_biquad_lanes packs 64 jobs per wave
  add("", 8, true, 32, 256, 32, 70, 1);
  // the last piece 1, 3, 4 and 31 frames beyond a multiple of 32: the planner never cuts so, no launcher forbids it
  for (int k : {1, 3, 8})
    for (int r : {1, 3, 4, 31}) {
      cases.push_back(PipeCase{fmt("pipe.ragged.s%d.r%d", k, r), k, true, 64, 3, 32 + r, 33, 1, false});
    }
  for (const PipeCase& pc : cases) pipe_case(pc);
}

int main(int argc, char** argv) {
  const std::string fam = argc > 1 ? argv[1] : "";
  if (fam == "scan") family_scan();
  else if (fam == "expand") family_expand();
  else if (fam == "pipe") family_pipe();
  else {
    std::printf("usage: biquad_split_check scan|expand|pipe\n");
    return 2;
  }
  std::printf("%s\n", failures ? "FAILED" : "all ok");
  return failures ? 1 : 0;
}
