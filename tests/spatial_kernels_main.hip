// Stand-alone run of the four SpatialPannerNode kernels of graphaudio_amd/csrc/ga_spatial.hip through their launchers alone, on plain
// device tables, against tests/spatial_ref.hpp (the contracts of ga_kernels.hpp and DESIGN.md section 2e in float64 and as the float32
// chain the header promises).  The node has no counterpart in the reference, so nothing else says these bits are right.  argv[1]
// picks a family:
//   panner  spatial_panner_kernel on inputs on which float32 in any order is float64 (x integers in [-3, 3], taps integers in
//           [-2, 2], w one of (1,0,0,0), (1/2,1/2,0,0), (1/2,0,1/2,0), (1/4,1/4,1/4,1/4), gb 1/2, 1 or 2, dry 0, 1/2 or 1): m is a
//           multiple of 1/2, F of 1/8 with |F| <= 4, a sum over 512 taps plus the dry term at most 6147 in units of 1/16, after the
//           fade in units of 1/2048, and 6147 * 2048 < 2^24.  The program recomputes sum |F||m| + |dry x| per sample from the drawn
//           data and refuses a case outside that budget.  got == (float)ref64 on every written sample and on all 512 history samples.
//   float   the same kernel on uniform data: bits equal form (b), and per sample
//             |got - ref64| <= gamma_c (w_n (sum_k |F_k||m_{n-k}| + |dry x|) + (1 - w_n) (the same of the previous filters)),
//           gamma_c = c u / (1 - c u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Lemma 3.1).
//           c counts the roundings a term can pass through: 5 for a filter tap (four fma in q, then gb *; the four taps that meet do
//           not cancel in these scenes, so the five are relative to |F_k|), 1 for a stereo block's mix (the sum; the halving is
//           exact), T for the fma chain (term k passes T - k of them, the first term all T), 1 for fma(dry, x, sum), and while
//           fading 1 for the product with 1 - w_n (w_n and 1 - w_n are exact) and 1 for the final fma: c = T + 9.
//   direct  spatial_direct_kernel bit for bit against the host walk of ga_spatial_direct.hpp (spatial_ref.hpp, direct_walk)
//   desc    spatial_desc_kernel against spatial_geometry<SpatialMathDouble>, spatial_occlusion and spatial_differs on the host: idx
//           and the fade bit equal, w within one float32 ulp, gb / dry bit for bit with the cones off and the linear or inverse
//           model and within 1e-6 relative otherwise; seg, the other flag bits, entry 0 (unless the contract writes it) and every
//           other table entry untouched.  A case within 1e-6 of an integer in pa or pe, 1e-4 of 0.999 in the directivity or below
//           0.01 in distance is refused.
//   head    spatial_head_kernel: every tap within max(one float32 ulp at the value, 2^-40) of spatial_head_tap on the host
// Every output array lies between two guard regions of 0xCD and is born 0xCD: the guards must be untouched, what the contract says
// is written must be right, everything else must still read 0xCD.  Inputs lie between NaN guards, and every input element the
// contract does not read is NaN (the rows of a segment outside its blocks, the gap behind a channel's taps, a modulation input
// behind sample 0 of a block).  Job tables are checked against the contract before anything is launched; a case outside it is
// reported as failed and not run.  Each check prints "check <name> ok|FAIL <figures> [wall time since the previous line]"; exit
// status 1 if any check fails, 3 at once after a HIP error (the caller then starts nothing more).
// tests/test_gpu_spatial_kernels.py holds the set of check names.
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
#include "spatial_ref.hpp"

using namespace ga;
namespace sr = spatial_ref;
static_assert(sr::kBlock == kBlock && sr::kMaxTaps == kSpatialMaxTaps && sr::kRun == kSpatialRun, "tests/spatial_ref.hpp restates the block length, the tap limit and the run length");
static_assert(sizeof(sr::Desc) == sizeof(SpatialDesc) && sizeof(sr::Work) == sizeof(SpatialWork), "tests/spatial_ref.hpp restates SpatialDesc and SpatialWork");
static_assert(6147 * 2048 < (1 << 24), "the exactness budget of the panner family");

namespace ga {
[[noreturn]] void launch_fail(const char* what) {   // (ga_engine.cpp's is not linked here)
  std::printf("launch_fail: %s\n", what);
  std::exit(2);
}
}  // namespace ga

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); std::fflush(stdout); std::exit(3); } } while (0)

static int failures = 0;
static void check(const std::string& name, bool ok, const char* fmt, ...) {
  char buf[1536];
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
  char buf[512];
  va_list ap;
  va_start(ap, f);
  std::vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
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
static const float kCDf = from_bits(kCD);

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
  uint8_t* b(size_t byte_off = 0) const { return (uint8_t*)(raw + g) + byte_off; }
  void upload(const void* src, size_t n, size_t byte_off = 0) { CK(hipMemcpy(raw + g + byte_off, src, n, hipMemcpyHostToDevice)); }
  std::vector<float> host(size_t nfloats) const {
    std::vector<float> h(nfloats);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h.data(), raw + g, nfloats * 4, hipMemcpyDeviceToHost));
    return h;
  }
  std::vector<uint8_t> host_bytes(size_t n) const {
    std::vector<uint8_t> h(n);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h.data(), raw + g, n, hipMemcpyDeviceToHost));
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
template <class T>
static size_t append(std::vector<uint8_t>& tb, const T* p, size_t n) {   // -> the byte offset, 16-byte aligned
  tb.resize((tb.size() + 15) / 16 * 16);
  const size_t off = tb.size();
  tb.resize(off + n * sizeof(T));
  if (n) std::memcpy(tb.data() + off, p, n * sizeof(T));
  return off;
}

// =====================================================================================================================
//  panner / float
// =====================================================================================================================
static const double kU = 5.9604644775390625e-08;   // 2^-24

struct PannerRig {
  std::vector<const sr::NodeScene*> nodes;
  std::vector<const sr::HrirSet*> sets;
  std::vector<std::unique_ptr<GuardedIn>> dsets, din;
  std::unique_ptr<Guarded> out, hist;
  std::vector<size_t> out_off;
  int slots;
  PannerRig(const std::vector<const sr::NodeScene*>& nodes_, int launches) : nodes(nodes_), slots(launches + 1) {
    size_t total = 0;
    for (const sr::NodeScene* S : nodes) {
      if (std::find(sets.begin(), sets.end(), S->set) == sets.end()) {
        sets.push_back(S->set);
        dsets.emplace_back(new GuardedIn(S->set->h));
      }
      din.emplace_back(new GuardedIn(S->in));
      out_off.push_back(total);
      total += (size_t)(2 * S->n * kBlock);
    }
    out.reset(new Guarded(total * 4));
    hist.reset(new Guarded(nodes.size() * (size_t)slots * kSpatialMaxTaps * 4));
    reset();
  }
  void reset() {
    out->reset();
    hist->reset();
    for (size_t j = 0; j < nodes.size(); j++) hist->upload(nodes[j]->hist.data(), kSpatialMaxTaps * 4, j * (size_t)slots * kSpatialMaxTaps * 4);
  }
  const float* set_dev(const sr::HrirSet* s) const { return dsets[(size_t)(std::find(sets.begin(), sets.end(), s) - sets.begin())]->f(); }
  // launch number li: blocks [g0, g1) of every node (g1 < 0: every node whole).  false: the tables are outside the contract
  bool launch(int li, int64_t g0, int64_t g1, bool span, sr::Rng& rng, std::string& why) {
    std::vector<uint8_t> tb;
    std::vector<SpatialJob> jobs;
    std::vector<sr::Work> works;
    std::vector<sr::Node> slices;
    std::vector<std::vector<sr::Seg>> segstore(nodes.size());
    for (size_t j = 0; j < nodes.size(); j++) {
      const sr::NodeScene& S = *nodes[j];
      const int64_t len = (g1 < 0 ? S.n : g1) - g0, N = S.n * kBlock;
      if (len < 1 || g0 + len > S.n) {
        why = "the cut lies outside the node";
        return false;
      }
      slices.push_back(sr::slice_node(S, g0, len, S.hist.data(), segstore[j]));
      std::vector<SpatialSeg> segs;
      for (size_t s = 0; s < S.off_l.size(); s++)
        segs.push_back(SpatialSeg{din[j]->f((size_t)S.off_l[s]) + g0 * kBlock, S.off_r[s] < 0 ? nullptr : din[j]->f((size_t)S.off_r[s]) + g0 * kBlock});
      SpatialJob job{};
      job.hrir = set_dev(S.set);
      job.hstride = S.set->hstride;
      job.desc_off = append(tb, S.desc.data() + g0, (size_t)len + 1);
      job.seg_off = append(tb, segs.data(), segs.size());
      job.hist_in = hist->f((j * (size_t)slots + (size_t)li) * kSpatialMaxTaps);
      job.hist_out = hist->f((j * (size_t)slots + (size_t)li + 1) * kSpatialMaxTaps);
      job.out_l = out->f(out_off[j] + (size_t)(g0 * kBlock));
      job.out_r = out->f(out_off[j] + (size_t)(N + g0 * kBlock));
      job.nblocks = len;
      job.taps = S.set->taps;
      jobs.push_back(job);
      const std::vector<sr::Work> w = span ? sr::span_works(len, (int)j) : sr::plan_works(slices.back().desc, len, (int)j);
      works.insert(works.end(), w.begin(), w.end());
    }
    for (size_t i = works.size(); i > 1; i--) std::swap(works[i - 1], works[(size_t)rng.below((int)i)]);   // the order of the workgroups is no part of the contract
    if (const char* f = sr::panner_facts(slices.data(), (int)slices.size(), works.data(), (int)works.size())) {
      why = f;
      return false;
    }
    Guarded dtb(tb.size(), kNaN);
    dtb.upload(tb.data(), tb.size());
    DevIn<SpatialJob> djobs(jobs);
    std::vector<SpatialWork> gw(works.size());
    std::memcpy(gw.data(), works.data(), works.size() * sizeof(SpatialWork));
    DevIn<SpatialWork> dworks(gw);
    launch_spatial_panner(nullptr, dworks.p, (int)gw.size(), djobs.p, dtb.b());
    sync_check();
    return true;
  }
};

struct PannerWant {   // per node: the expected bits
  std::vector<float> out[2];
  std::vector<char> written;
  std::vector<float> mixed;   // [512 + N]: the history and m
  sr::Rendered<double> a;
};
// exact: (float) of form (a), after the budget check; otherwise form (b)
static bool panner_want(const sr::NodeScene& S, bool exact, PannerWant& W, std::string& why, double& worst_mag) {
  const sr::Node nd = S.node();
  W.a = sr::render64(nd);
  const sr::Rendered<float> b = sr::render32(nd);
  W.written = W.a.written;
  const size_t N = (size_t)(S.n * kBlock);
  W.mixed = S.hist;
  for (size_t f = 0; f < N; f++) W.mixed.push_back(sr::mix32(nd, (int64_t)f));
  for (int e = 0; e < 2; e++) {
    W.out[e].resize(N);
    for (size_t f = 0; f < N; f++) W.out[e][f] = exact ? (float)W.a.out[e][f] : b.out[e][f];
  }
  if (!exact) return true;
  auto on = [](float v, float step, float lim) { return v != v || (std::fabs(v) <= lim && v / step == std::floor(v / step)); };
  bool ok = true;
  for (float v : S.in) ok = ok && on(v, 1.f, 3.f);
  for (float v : S.hist) ok = ok && v == v && on(v, .5f, 3.f);
  for (float v : S.set->h) ok = ok && on(v, 1.f, 2.f);
  for (const sr::Desc& d : S.desc) {
    float sum = 0.f;
    for (int q = 0; q < 4; q++) {
      ok = ok && (d.w[q] == 0.f || d.w[q] == .25f || d.w[q] == .5f || d.w[q] == 1.f);
      sum += d.w[q];
    }
    ok = ok && sum == 1.f && (d.gb == .5f || d.gb == 1.f || d.gb == 2.f) && (d.dry == 0.f || d.dry == .5f || d.dry == 1.f);
  }
  for (int e = 0; e < 2; e++)
    for (size_t f = 0; f < N; f++) {
      worst_mag = std::max(worst_mag, W.a.mag[e][f]);
      ok = ok && (double)W.out[e][f] == W.a.out[e][f];
    }
  for (size_t f = 0; f < N; f++) ok = ok && (double)W.mixed[kSpatialMaxTaps + f] == sr::mix64(nd, (int64_t)f);
  if (!ok || !(worst_mag * 2048.0 < 16777216.0)) {
    why = "the drawn data is outside the exactness budget";
    return false;
  }
  return true;
}

struct PannerTally {
  size_t written = 0, wrong = 0, stray = 0, hist_wrong = 0, hist_stray = 0, guards = 0;
  double ratio = 0.0, ratio_host = 0.0;
  std::string first;
  bool ok() const { return !wrong && !stray && !hist_wrong && !hist_stray && !guards; }
};
// the device's arrays after the launches whose cuts are `cuts` (block numbers, cuts[0] = 0 ... the chunk's end)
static void panner_compare(const PannerRig& rig, const std::vector<PannerWant>& want, const std::vector<int64_t>& cuts, bool exact, PannerTally& t, std::vector<float>* keep = nullptr) {
  size_t total = 0;
  for (const sr::NodeScene* S : rig.nodes) total += (size_t)(2 * S->n * kBlock);
  const std::vector<float> got = rig.out->host(total), gh = rig.hist->host(rig.nodes.size() * (size_t)rig.slots * kSpatialMaxTaps);
  if (keep) *keep = got;
  for (size_t j = 0; j < rig.nodes.size(); j++) {
    const sr::NodeScene& S = *rig.nodes[j];
    const PannerWant& W = want[j];
    const size_t N = (size_t)(S.n * kBlock);
    const double c = S.set->taps + 9, gamma = c * kU / (1.0 - c * kU);
    for (int e = 0; e < 2; e++)
      for (size_t f = 0; f < N; f++) {
        const float g = got[rig.out_off[j] + (size_t)e * N + f];
        if (!W.written[f / kBlock]) {
          t.stray += !is_cd(g);
          continue;
        }
        t.written++;
        const bool same = exact ? g == W.out[e][f] : bits(g) == bits(W.out[e][f]);
        if (!same && !t.wrong++) t.first = fmt("node %zu ear %d block %zu n %zu got %.9g want %.9g", j, e, f / kBlock, f % kBlock, (double)g, (double)W.out[e][f]);
        const double den = gamma * W.a.mag[e][f];
        auto rat = [&](float v) { const double r = std::fabs((double)v - W.a.out[e][f]); return r == 0.0 ? 0.0 : (r == r ? r / den : 1e300); };
        t.ratio = std::max(t.ratio, rat(g));
        t.ratio_host = std::max(t.ratio_host, rat(W.out[e][f]));
      }
    for (int s = 1; s < rig.slots; s++) {   // slot s: the history behind launch s - 1
      const bool made = (size_t)s < cuts.size();
      const size_t g1 = made ? (size_t)((cuts[(size_t)s] < 0 ? S.n : cuts[(size_t)s]) * kBlock) : 0;
      for (size_t i = 0; i < (size_t)kSpatialMaxTaps; i++) {
        const float g = gh[(j * (size_t)rig.slots + (size_t)s) * kSpatialMaxTaps + i];
        if (!made) t.hist_stray += !is_cd(g);
        else if (!(g == W.mixed[g1 + i]) && !t.hist_wrong++ && t.first.empty()) t.first = fmt("node %zu history %d sample %zu got %.9g want %.9g", j, s, i, (double)g, (double)W.mixed[g1 + i]);
      }
    }
  }
  t.guards += rig.out->guard_damage() + rig.hist->guard_damage();
  for (const auto& d : rig.din) t.guards += d->guard_damage();
  for (const auto& d : rig.dsets) t.guards += d->guard_damage();
}

// one check: the nodes through each of the cut lists in turn (every list: one launch per piece), every render held to the
// reference and to the first render's bits
static void panner_case(const std::string& name, const std::vector<const sr::NodeScene*>& nodes, const std::vector<std::vector<int64_t>>& cutlists, bool span, bool exact, uint64_t seed) {
  std::vector<PannerWant> want(nodes.size());
  std::string why;
  double worst_mag = 0.0;
  for (size_t j = 0; j < nodes.size(); j++)
    if (!panner_want(*nodes[j], exact, want[j], why, worst_mag)) {
      check(name, false, "refused: %s (largest sum |F||m| + |dry x| %.1f)", why.c_str(), worst_mag);
      return;
    }
  size_t launches = 1;
  for (const auto& c : cutlists) launches = std::max(launches, c.size() - 1);
  PannerRig rig(nodes, (int)launches);
  sr::Rng rng{seed};
  PannerTally t;
  std::vector<float> first, again;
  size_t differ = 0;
  for (size_t c = 0; c < cutlists.size(); c++) {
    if (c) rig.reset();
    const std::vector<int64_t>& cuts = cutlists[c];
    for (size_t li = 0; li + 1 < cuts.size(); li++)
      if (!rig.launch((int)li, cuts[li], cuts[li + 1], span, rng, why)) {
        check(name, false, "refused: %s", why.c_str());
        return;
      }
    panner_compare(rig, want, cuts, exact, t, c ? &again : &first);
    if (c)
      for (size_t i = 0; i < first.size(); i++) differ += bits(first[i]) != bits(again[i]);
  }
  const bool ok = t.ok() && differ == 0 && t.written > 0;
  if (exact)
    check(name, ok, "written %zu wrong %zu, unwritten not 0xCD %zu, history wrong %zu stray %zu, guards %zu, between cuts %zu, largest sum %.1f (budget 8192)%s%s",
          t.written, t.wrong, t.stray, t.hist_wrong, t.hist_stray, t.guards, differ, worst_mag, t.first.empty() ? "" : " first: ", t.first.c_str());
  else
    check(name, ok && t.ratio <= 1.0 && t.ratio == t.ratio_host,
          "written %zu not form (b)'s bits %zu, ratio to gamma_c bound %.4f (form (b) on the host %.4f), unwritten not 0xCD %zu, history wrong %zu stray %zu, guards %zu%s%s",
          t.written, t.wrong, t.ratio, t.ratio_host, t.stray, t.hist_wrong, t.hist_stray, t.guards, t.first.empty() ? "" : " first: ", t.first.c_str());
}

static const int kPannerT[8] = {1, 2, 3, 127, 128, 129, 511, 512};
static void family_panner() {
  uint64_t seed = 0x5A710000u;
  // T x chunk length: three nodes in one launch, two of them on one set; works as planSpatialPanner cuts them: runs of (1, 2), (3, 1),
  // (4, 1), (4, 2, 3) blocks follow from the segments
  struct { int n; const char* mixed; } const kLen[5] = {{1, "s"}, {3, "mss"}, {4, "mmms"}, {5, "sssss"}, {9, "mmmmmmsss"}};
  for (int T : kPannerT)
    for (const auto& L : kLen) {
      sr::Rng rng{seed++};
      const sr::HrirSet A = sr::make_hrir(rng, 6, T, T, true), B = sr::make_hrir(rng, 4, T, T + 5, true);   // (B: NaN in the gap behind the taps)
      sr::NodeScene n0, n1, n2;
      sr::make_node(n0, rng, A, L.mixed, sr::kFadeEvery, true, false, false);                         // mono and stereo segments, every block fades
      sr::make_node(n1, rng, A, std::string((size_t)L.n, 'm').c_str(), sr::kFadeNone, true, true, false);   // no fade anywhere, a history
      sr::make_node(n2, rng, B, std::string((size_t)L.n, 's').c_str(), sr::kFadeFirst, true, true, true);   // block 0 fades from entry 0; views offset by one float
      panner_case(fmt("panner.T%d.n%d", T, L.n), {&n0, &n1, &n2}, {{0, -1}}, false, true, seed);
    }
  // silent blocks at the start, inside and at the end of a run (works that span them), and the same chunk cut as the planner cuts it
  // (it ends on silence: a work of no blocks carries the history)
  for (int T : {3, 129, 512})
    for (int span = 0; span < 2; span++) {
      sr::Rng rng{seed++};
      const sr::HrirSet A = sr::make_hrir(rng, 6, T, T + 1, true);
      sr::NodeScene n0, n1;
      sr::make_node(n0, rng, A, "-mm-m-ss-", sr::kFadeEvery, true, true, false);
      sr::make_node(n1, rng, A, "s--ms-m", sr::kFadeEvery, true, true, true);
      panner_case(fmt("panner.silent.%s.T%d", span ? "span" : "plan", T), {&n0, &n1}, {{0, -1}}, span != 0, true, seed);
    }
  // the tail work reads hist_in to fill hist_out
  for (int n = 1; n <= 3; n++) {
    sr::Rng rng{seed++};
    const sr::HrirSet A = sr::make_hrir(rng, 6, 512, 512, true);
    sr::NodeScene n0;
    sr::make_node(n0, rng, A, std::string((size_t)n, n == 2 ? 's' : 'm').c_str(), sr::kFadeEvery, true, true, false);
    panner_case(fmt("panner.hist.T512.n%d", n), {&n0}, {{0, -1}}, false, true, seed);
  }
  // nine blocks as one chunk, as 4 + 5 and as 1 + 8: hist_out is the next launch's hist_in, entry 0 the previous chunk's last entry
  for (int T : {129, 512}) {
    sr::Rng rng{seed++};
    const sr::HrirSet A = sr::make_hrir(rng, 6, T, T, true);
    sr::NodeScene n0;
    sr::make_node(n0, rng, A, "mmmssmmss", sr::kFadeEvery, true, true, false);
    panner_case(fmt("panner.cut.T%d", T), {&n0}, {{0, 9}, {0, 4, 9}, {0, 1, 9}}, false, true, seed);
  }
}
static void family_float() {
  uint64_t seed = 0xF10A7000u;
  for (int T : {129, 512})
    for (int stereo = 0; stereo < 2; stereo++)
      for (int fade = 0; fade < 2; fade++) {
        sr::Rng rng{seed++};
        const sr::HrirSet A = sr::make_hrir(rng, 6, T, T + 2, false);
        sr::NodeScene n0;
        sr::make_node(n0, rng, A, stereo ? "sssss" : "mmmmm", fade ? sr::kFadeEvery : sr::kFadeNone, false, true, stereo != 0);
        panner_case(fmt("float.T%d.%s.%s", T, stereo ? "stereo" : "mono", fade ? "fade" : "steady"), {&n0}, {{0, -1}, {0, 2, 5}}, false, false, seed);
      }
}

// =====================================================================================================================
//  direct
// =====================================================================================================================
static const SpatialEq kIdentity{1.0f, 0.0f, 0.0f};
struct DJob {   // one job of a launch as the host states it
  int stereo, b0, nb;
  SpatialEq prev;
  int open, from_state, prev_valid;
};
struct DirectRig {   // `njobs` nodes over a chunk of `nblocks` blocks; rows and states persist from launch to launch
  int njobs, nblocks;
  size_t N;
  std::vector<float> x;                          // [job][ch][N]
  std::vector<std::vector<SpatialEq>> eqs;       // per job: entry b + 1 = block b
  std::vector<float> want;                       // [job][ch][N], born 0xCD
  std::vector<sr::DirectState> wst;              // the expected states
  std::unique_ptr<GuardedIn> din;
  std::unique_ptr<Guarded> dout, dst, dtb;
  std::vector<uint64_t> eq_off;
  SpatialBands K = spatial_bands(48000.0);
  DirectRig(int njobs_, int nblocks_, sr::Rng& rng, const std::vector<std::vector<SpatialEq>>& eqs_, const std::vector<sr::DirectState>& st0)
      : njobs(njobs_), nblocks(nblocks_), N((size_t)nblocks_ * kBlock), eqs(eqs_), wst(st0) {
    x.resize((size_t)njobs * 2 * N);
    for (float& v : x) v = rng.unit();
    want.assign(x.size(), kCDf);
    din.reset(new GuardedIn(x));
    dout.reset(new Guarded(x.size() * 4));
    std::vector<SpatialDirectState> st((size_t)njobs);
    for (int j = 0; j < njobs; j++) {
      std::memset(&st[(size_t)j], 0xCD, sizeof(SpatialDirectState));
      for (int ch = 0; ch < 2; ch++) {
        st[(size_t)j].zl[ch] = st0[(size_t)j].zl[ch];
        st[(size_t)j].zh[ch] = st0[(size_t)j].zh[ch];
        st[(size_t)j].open[ch] = st0[(size_t)j].open[ch];
      }
      st[(size_t)j].prev = st0[(size_t)j].prev;
    }
    dst.reset(new Guarded(st.size() * sizeof(SpatialDirectState)));
    dst->upload(st.data(), st.size() * sizeof(SpatialDirectState));
    std::vector<uint8_t> tb;
    for (int j = 0; j < njobs; j++) {
      std::vector<SpatialEqEntry> e((size_t)nblocks + 1);
      std::memset(e.data(), 0xFF, e.size() * sizeof(SpatialEqEntry));   // (entry 0 is not used: NaN)
      for (int b = 1; b <= nblocks; b++) e[(size_t)b].c = eqs[(size_t)j][(size_t)b];
      eq_off.push_back(append(tb, e.data(), e.size()));
    }
    dtb.reset(new Guarded(tb.size(), kNaN));
    dtb->upload(tb.data(), tb.size());
  }
  // one launch over the first jobs.size() nodes; the inputs outside a job's blocks are not NaN here (the rows are whole), the outputs
  // outside them must stay 0xCD
  bool launch(const std::vector<DJob>& jobs, std::string& why) {
    std::vector<SpatialDirectJob> gj;
    int max_nb = 0;
    for (size_t j = 0; j < jobs.size(); j++) {
      const DJob& d = jobs[j];
      if ((int)j >= njobs || d.nb < 1 || d.b0 < 0 || d.b0 + d.nb > nblocks) {
        why = "b0 / nb outside the chunk";
        return false;
      }
      max_nb = std::max(max_nb, d.nb);
      SpatialDirectJob g{};
      for (int ch = 0; ch < (d.stereo ? 2 : 1); ch++) {
        g.in[ch] = din->f((j * 2 + (size_t)ch) * N);
        g.out[ch] = dout->f((j * 2 + (size_t)ch) * N);
      }
      g.eq_off = eq_off[j];
      g.state = (SpatialDirectState*)dst->b(j * sizeof(SpatialDirectState));
      g.prev = d.prev;
      g.open = d.open;
      g.from_state = d.from_state;
      g.prev_valid = d.prev_valid;
      g.b0 = d.b0;
      g.nb = d.nb;
      gj.push_back(g);
      sr::DirectJob r{{x.data() + j * 2 * N, d.stereo ? x.data() + (j * 2 + 1) * N : nullptr}, {want.data() + j * 2 * N, d.stereo ? want.data() + (j * 2 + 1) * N : nullptr},
                      eqs[j].data(), d.prev, d.open, d.from_state, d.prev_valid, d.b0, d.nb};
      sr::direct_walk(K, r, wst[j]);
    }
    DevIn<SpatialDirectJob> dj(gj);
    launch_spatial_direct(nullptr, dj.p, (int)gj.size(), max_nb, dtb->b(), K);
    sync_check();
    return true;
  }
  // -> figures; zl / zh are the contract's where the run is open
  bool compare(std::string& figures, std::vector<float>* keep = nullptr) {
    const std::vector<float> got = dout->host(x.size());
    if (keep) *keep = got;
    const std::vector<uint8_t> sb = dst->host_bytes((size_t)njobs * sizeof(SpatialDirectState));
    size_t wrong = 0, stray = 0, written = 0, st_wrong = 0;
    std::string first;
    for (size_t i = 0; i < got.size(); i++) {
      if (is_cd(want[i])) {
        stray += !is_cd(got[i]);
        continue;
      }
      written++;
      if (bits(got[i]) != bits(want[i]) && !wrong++) first = fmt(" first: job %zu ch %zu block %zu n %zu got %.9g want %.9g", i / (2 * N), i / N % 2, i % N / kBlock, i % kBlock, (double)got[i], (double)want[i]);
    }
    for (int j = 0; j < njobs; j++) {
      SpatialDirectState s;
      std::memcpy(&s, sb.data() + (size_t)j * sizeof s, sizeof s);
      const sr::DirectState& w = wst[(size_t)j];
      size_t bad = 0;
      for (int ch = 0; ch < 2; ch++) {
        bad += s.open[ch] != w.open[ch];
        if (w.open[ch]) bad += bits(s.zl[ch]) != bits(w.zl[ch]) || bits(s.zh[ch]) != bits(w.zh[ch]);
      }
      bad += bits(s.prev.cM) != bits(w.prev.cM) || bits(s.prev.cL) != bits(w.prev.cL) || bits(s.prev.cH) != bits(w.prev.cH);
      bad += (uint32_t)s.pad_ != kCD;
      if (bad && !st_wrong) first += fmt(" state of job %d: open %d %d want %d %d", j, s.open[0], s.open[1], w.open[0], w.open[1]);
      st_wrong += bad;
    }
    const size_t guards = dout->guard_damage() + dst->guard_damage() + din->guard_damage() + dtb->guard_damage();
    figures = fmt("written %zu wrong %zu, unwritten not 0xCD %zu, state fields wrong %zu, guards %zu", written, wrong, stray, st_wrong, guards) + first;
    return written > 0 && !wrong && !stray && !st_wrong && !guards;
  }
};
static SpatialEq draw_eq(sr::Rng& rng) { return SpatialEq{0.6f + 0.4f * rng.unit(), 0.5f * rng.unit(), 0.5f * rng.unit()}; }
// kind 0: the identity throughout; 1: active from block 0; 2: identity, active, identity, identity, active ... (a block behind an
// active one is active too: two identities close the run); 3: drawn per block, one in three the identity
static std::vector<SpatialEq> draw_eqs(sr::Rng& rng, int nblocks, int kind) {
  std::vector<SpatialEq> e((size_t)nblocks + 1, kIdentity);
  for (int b = 0; b < nblocks; b++) {
    const bool act = kind == 1 || (kind == 2 && b % 4 == 1) || (kind == 3 && rng.below(3) != 0);
    if (act) e[(size_t)b + 1] = draw_eq(rng);
  }
  return e;
}
static sr::DirectState draw_state(sr::Rng& rng, int open) {
  sr::DirectState s{};
  for (int ch = 0; ch < 2; ch++) {
    s.zl[ch] = 0.25f * rng.unit();
    s.zh[ch] = 0.25f * rng.unit();
    s.open[ch] = (open >> ch) & 1;
  }
  s.prev = draw_eq(rng);
  return s;
}
static void direct_single(const std::string& name, uint64_t seed, int nblocks, int kind, int stereo, const DJob& proto, int state_open, bool expect_copy) {
  sr::Rng rng{seed};
  const std::vector<std::vector<SpatialEq>> eqs{draw_eqs(rng, nblocks, kind)};
  DirectRig rig(1, nblocks, rng, eqs, {draw_state(rng, state_open)});
  DJob j = proto;
  j.stereo = stereo;
  std::string why, figures;
  if (!rig.launch({j}, why)) {
    check(name, false, "refused: %s", why.c_str());
    return;
  }
  bool ok = rig.compare(figures);
  if (expect_copy) {   // the identity throughout: out is in, bit for bit, and the run ends closed
    for (size_t i = 0; i < rig.x.size(); i++)
      if (!is_cd(rig.want[i])) ok = ok && bits(rig.want[i]) == bits(rig.x[i]);
    ok = ok && rig.wst[0].open[0] == 0 && rig.wst[0].open[1] == 0;
  }
  check(name, ok, "%s", figures.c_str());
}
static void family_direct() {
  uint64_t seed = 0xD14EC700u;
  // njobs = 1, 8, 9 (a second workgroup with one job): mono and stereo jobs mixed, nb and b0 differing per job, every kind of triple
  // table, prev_valid and from_state both ways, open runs carried in through the job and through the state
  for (int njobs : {1, 8, 9}) {
    sr::Rng rng{seed++};
    const int nblocks = 9;
    std::vector<std::vector<SpatialEq>> eqs;
    std::vector<sr::DirectState> st;
    std::vector<DJob> jobs;
    for (int j = 0; j < njobs; j++) {
      eqs.push_back(draw_eqs(rng, nblocks, (j + 1) % 4));
      DJob d{};
      d.stereo = j % 2;
      d.b0 = j % 3;
      d.nb = njobs == 1 ? 5 : 1 + (j * 5) % 7;   // 1, 6, 4, 2, 7, 5, 3, 1, 6
      d.prev_valid = j % 4 != 2;
      d.from_state = (j / 2) % 2;
      d.open = j % 4;
      d.prev = j % 3 ? draw_eq(rng) : kIdentity;
      st.push_back(draw_state(rng, 3 - j % 4));
      jobs.push_back(d);
    }
    DirectRig rig(njobs, nblocks, rng, eqs, st);
    std::string why, figures;
    if (!rig.launch(jobs, why)) {
      check(fmt("direct.n%d", njobs), false, "refused: %s", why.c_str());
      continue;
    }
    const bool ok = rig.compare(figures);
    check(fmt("direct.n%d", njobs), ok, "%s", figures.c_str());
  }
  const DJob fresh{0, 0, 9, kIdentity, 0, 0, 0};
  direct_single("direct.identity.mono", seed++, 9, 0, 0, fresh, 3, true);
  direct_single("direct.identity.stereo", seed++, 9, 0, 1, DJob{0, 0, 9, kIdentity, 0, 0, 1}, 0, true);
  direct_single("direct.active0", seed++, 9, 1, 1, fresh, 3, false);
  direct_single("direct.restart", seed++, 9, 2, 1, fresh, 0, false);           // identity -> active -> identity -> active: the second run from zero state
  {
    sr::Rng rng{seed++};
    const SpatialEq carried = draw_eq(rng);
    direct_single("direct.carry_job", seed++, 9, 1, 1, DJob{0, 2, 5, carried, 3, 0, 1}, 0, false);       // an open run through the job (the state's flags say closed)
    direct_single("direct.carry_job_half", seed++, 9, 1, 1, DJob{0, 2, 5, carried, 2, 0, 1}, 1, false);  // ... open on channel 1 alone
    direct_single("direct.carry_state", seed++, 9, 3, 1, DJob{0, 1, 8, kIdentity, 0, 1, 1}, 3, false);   // ... through the state (the job's say closed)
    direct_single("direct.prev_invalid", seed++, 9, 1, 1, DJob{0, 0, 9, carried, 3, 1, 0}, 3, false);    // no previous block: nothing carried counts
  }
  // one launch of 9 blocks against 4 + 5, the cut inside an open run: the same bits
  {
    sr::Rng rng{seed++};
    std::vector<SpatialEq> e((size_t)10, kIdentity);
    for (int b : {1, 2, 3, 4, 5, 7}) e[(size_t)b + 1] = draw_eq(rng);
    const std::vector<std::vector<SpatialEq>> eqs{e};
    const sr::DirectState st0 = draw_state(rng, 0);
    sr::Rng r1 = rng, r2 = rng;
    DirectRig one(1, 9, r1, eqs, {st0}), two(1, 9, r2, eqs, {st0});
    std::string why, f1, f2;
    std::vector<float> g1, g2;
    bool ok = one.launch({DJob{1, 0, 9, kIdentity, 0, 1, 0}}, why) && two.launch({DJob{1, 0, 4, kIdentity, 0, 1, 0}}, why);
    ok = ok && two.wst[0].open[0] == 1 && two.launch({DJob{1, 4, 5, kIdentity, 0, 1, 1}}, why);
    if (!ok) {
      check("direct.cut", false, "refused: %s", why.c_str());
    } else {
      ok = one.compare(f1, &g1);
      ok = two.compare(f2, &g2) && ok;
      size_t differ = 0;
      for (size_t i = 0; i < g1.size(); i++) differ += bits(g1[i]) != bits(g2[i]);
      check("direct.cut", ok && !differ, "one piece: %s; 4 + 5: %s; between them %zu", f1.c_str(), f2.c_str(), differ);
    }
  }
}

// =====================================================================================================================
//  desc
// =====================================================================================================================
enum { kPrevNone = 0, kPrevHost = 1, kPrevIn = 2 };
struct DSpec {   // one job
  int nblocks = 0, b0 = 0, nb = 0, A = 8, D = 40, model = kSpatialInverse;
  bool occlusion = false, exact_gain = true;
  int prev = kPrevNone;
  SpatialCarry carry{};                     // what the previous processed block left (host or device record)
  float value[kSpatialParams];
  std::vector<float> curve[kSpatialParams]; // [nblocks] or empty
  std::vector<float> mod[kSpatialParams];   // [nblocks]: sample 0 of every block, or empty
  float vmin[kSpatialParams], vmax[kSpatialParams];
  int seg0 = 5, flags0 = 3;                 // what the host left in seg and flags of every entry
};
static void desc_defaults(DSpec& s, sr::Rng& rng) {
  const float v[kSpatialParams] = {1.5f + rng.unit(), 0.75f * rng.unit(), -2.0f + rng.unit(), 1.f, 0.f, 0.f, 1.f, 100.f, 1.f, 360.f, 360.f, 0.f, 0.75f, 0.f, 1.f, 1.f, 1.f};
  for (int p = 0; p < kSpatialParams; p++) {
    s.value[p] = v[p];
    s.vmin[p] = -1000.f;
    s.vmax[p] = 1000.f;
  }
}
static const SpatialListener kListener{{0.125f, -0.25f, 0.375f, 0.8f, 0.f, 0.6f, 0.f, 1.f, 0.f, 0.6f, 0.f, -0.8f}};   // origin, right, up, ahead (an orthonormal frame, turned about y)

static uint32_t ulp_distance(float a, float b) {
  if (!(a == a) || !(b == b)) return bits(a) == bits(b) ? 0u : 0xFFFFFFFFu;
  const int32_t ia = (int32_t)bits(a), ib = (int32_t)bits(b);
  const int64_t la = ia < 0 ? (int64_t)INT32_MIN - ia : ia, lb = ib < 0 ? (int64_t)INT32_MIN - ib : ib;
  return (uint32_t)std::min<int64_t>(std::llabs(la - lb), 0xFFFFFFFFll);
}
struct DescTally {
  size_t blocks = 0, idx = 0, fade = 0, w = 0, gain = 0, host_fields = 0, eq = 0, stray = 0, carry = 0, entry0 = 0, guards = 0, fades_seen = 0, steady_seen = 0, gain_bits = 0;
  uint32_t w_ulp = 0;
  double gain_rel = 0.0;
  std::string first;
  bool ok() const { return blocks && !idx && !fade && !w && !gain && !host_fields && !eq && !stray && !carry && !entry0 && !guards; }
  std::string str() const {
    return fmt("blocks %zu (fading %zu), idx wrong %zu, fade bit wrong %zu, w beyond 1 ulp %zu (largest %u), gb / dry wrong %zu (not the host's bits %zu, largest relative %.2e), seg / flags touched %zu, EQ wrong %zu, ",
               blocks, fades_seen, idx, fade, w, w_ulp, gain, gain_bits, gain_rel, host_fields, eq) +
           fmt("entry 0 wrong %zu, carried record wrong %zu, other table bytes touched %zu, guards %zu", entry0, carry, stray, guards) + first;
  }
};
// the jobs of one launch on one table; carried records on the device: record 2 j is job j's prev_in, 2 j + 1 its prev_out
struct DescRig {
  std::vector<DSpec> specs;
  std::vector<uint8_t> tb0;      // the table as uploaded
  std::vector<size_t> desc_off, eq_off;
  std::vector<std::vector<size_t>> curve_off;
  std::unique_ptr<Guarded> dtb, dcarry;
  std::vector<std::unique_ptr<GuardedIn>> dmod;
  std::vector<std::vector<const float*>> mod_dev;
  explicit DescRig(const std::vector<DSpec>& specs_) : specs(specs_) {
    for (const DSpec& s : specs) {
      std::vector<SpatialDesc> d((size_t)s.nblocks + 1);
      std::memset(d.data(), 0xCD, d.size() * sizeof(SpatialDesc));
      for (SpatialDesc& e : d) {
        e.seg = s.seg0;
        e.flags = s.flags0;
      }
      desc_off.push_back(append(tb0, d.data(), d.size()));
      std::vector<SpatialEqEntry> q((size_t)s.nblocks + 1);
      std::memset(q.data(), 0xCD, q.size() * sizeof(SpatialEqEntry));
      eq_off.push_back(append(tb0, q.data(), q.size()));   // (the room is there whether the job names it or not: it must stay 0xCD)
      curve_off.emplace_back();
      mod_dev.emplace_back();
      for (int p = 0; p < kSpatialParams; p++) {
        curve_off.back().push_back(s.curve[p].empty() ? (size_t)-1 : append(tb0, s.curve[p].data(), s.curve[p].size()));
        const float* m = nullptr;
        if (!s.mod[p].empty()) {
          std::vector<float> sig((size_t)s.nblocks * kBlock, from_bits(kNaN));   // only sample 0 of a block of the job is read
          for (int b = s.b0; b < s.b0 + s.nb; b++) sig[(size_t)b * kBlock] = s.mod[p][(size_t)b];
          dmod.emplace_back(new GuardedIn(sig));
          m = dmod.back()->f();
        }
        mod_dev.back().push_back(m);
      }
    }
    dtb.reset(new Guarded(tb0.size()));
    dtb->upload(tb0.data(), tb0.size());
    dcarry.reset(new Guarded(specs.size() * 2 * sizeof(SpatialCarry)));
    for (size_t j = 0; j < specs.size(); j++)
      if (specs[j].prev == kPrevIn) dcarry->upload(&specs[j].carry, 40, j * 2 * sizeof(SpatialCarry));   // (the record's padding stays 0xCD)
  }
  void run(DescTally& t) {
    std::vector<SpatialDescJob> jobs;
    int max_nb = 0;
    for (size_t j = 0; j < specs.size(); j++) {
      const DSpec& s = specs[j];
      if (s.nb < 1 || s.b0 < 0 || s.b0 + s.nb > s.nblocks || s.A < 1 || s.D < s.A || s.D % s.A) {
        t.first = " refused: b0 / nb outside the chunk, or the set's shape";
        t.blocks = 0;
        return;
      }
      SpatialDescJob g{};
      g.desc_off = desc_off[j];
      g.b0 = s.b0;
      g.nb = s.nb;
      g.azimuths = s.A;
      g.dirs = s.D;
      g.model = s.model;
      g.prev_valid = s.prev != kPrevNone;
      g.prev_in = s.prev == kPrevIn ? (const SpatialCarry*)dcarry->b(j * 2 * sizeof(SpatialCarry)) : nullptr;
      g.prev_out = (SpatialCarry*)dcarry->b((j * 2 + 1) * sizeof(SpatialCarry));
      if (s.prev == kPrevHost) g.prev_host = s.carry;
      else std::memset(&g.prev_host, 0xFF, sizeof g.prev_host);   // (not to be read)
      for (int p = 0; p < kSpatialParams; p++) {
        g.value[p] = s.value[p];
        g.curve_off[p] = s.curve[p].empty() ? kSpatialNoCurve : (uint64_t)curve_off[j][(size_t)p];
        g.mod[p] = mod_dev[j][(size_t)p];
        g.vmin[p] = s.vmin[p];
        g.vmax[p] = s.vmax[p];
      }
      g.eq_off = s.occlusion ? (uint64_t)eq_off[j] : kSpatialNoCurve;
      jobs.push_back(g);
      max_nb = std::max(max_nb, s.nb);
    }
    // the expected table, and where the device may differ from it by a rounding
    std::vector<uint8_t> want = tb0;
    struct Loose { size_t off; int kind; bool exact; };   // kind 0: w (1 ulp), 1: gb / dry / g
    std::vector<Loose> loose;
    std::vector<SpatialCarry> wcarry(specs.size());
    for (size_t j = 0; j < specs.size(); j++) {
      const DSpec& s = specs[j];
      SpatialGeom pr{};
      bool have = s.prev != kPrevNone;
      if (have) {
        for (int q = 0; q < 4; q++) {
          pr.idx[q] = s.carry.idx[q];
          pr.w[q] = s.carry.w[q];
        }
        pr.g = s.carry.g;
        pr.beta = s.carry.beta;
        if (s.b0 == 0 && s.prev == kPrevIn) {   // entry 0 from the carried record: float32 operations on given values, bit for bit
          sr::Desc d0;
          std::memcpy(&d0, want.data() + desc_off[j], sizeof d0);
          sr::desc_fill(pr, s.D, d0);
          std::memcpy(want.data() + desc_off[j], &d0, sizeof d0);
        }
      }
      for (int b = s.b0; b < s.b0 + s.nb; b++) {
        float pv[kSpatialParams];
        for (int p = 0; p < kSpatialParams; p++)
          pv[p] = sr::krate(s.curve[p].empty() ? s.value[p] : s.curve[p][(size_t)b], s.mod[p].empty() ? nullptr : &s.mod[p][(size_t)b], s.vmin[p], s.vmax[p]);
        const sr::DescMargins mg = sr::desc_margins(pv, kListener.v, s.A, s.D);
        if (!sr::desc_margins_ok(mg)) {
          t.first = fmt(" refused: job %zu block %d sits at a jump of the definition (pa %.2e pe %.2e directivity %.2e distance %.3f)", j, b, mg.pa, mg.pe, mg.directivity, mg.distance);
          t.blocks = 0;
          return;
        }
        SpatialGeom cur;
        SpatialEq eq;
        sr::desc_block(pv, kListener.v, s.model, s.A, s.D, s.occlusion, cur, eq);
        const bool fade = have && spatial_differs(pr, cur);
        t.fades_seen += fade;
        t.steady_seen += have && !fade;
        const size_t off = desc_off[j] + (size_t)(b + 1) * sizeof(SpatialDesc);
        sr::Desc d;
        std::memcpy(&d, want.data() + off, sizeof d);
        sr::desc_fill(cur, s.D, d);
        d.flags = (d.flags & ~1) | (fade ? 1 : 0);
        std::memcpy(want.data() + off, &d, sizeof d);
        for (int q = 0; q < 4; q++) loose.push_back(Loose{off + offsetof(SpatialDesc, w) + 4 * (size_t)q, 0, false});
        loose.push_back(Loose{off + offsetof(SpatialDesc, gb), 1, s.exact_gain});
        loose.push_back(Loose{off + offsetof(SpatialDesc, dry), 1, s.exact_gain});
        if (s.occlusion) {
          SpatialEqEntry e;
          std::memcpy(&e, want.data() + eq_off[j] + (size_t)(b + 1) * sizeof e, sizeof e);
          e.c = eq;
          std::memcpy(want.data() + eq_off[j] + (size_t)(b + 1) * sizeof e, &e, sizeof e);
        }
        pr = cur;
        have = true;
        t.blocks++;
      }
      std::memset(&wcarry[j], 0xCD, sizeof(SpatialCarry));
      for (int q = 0; q < 4; q++) {
        wcarry[j].idx[q] = pr.idx[q];   // unclamped
        wcarry[j].w[q] = pr.w[q];
      }
      wcarry[j].g = pr.g;
      wcarry[j].beta = pr.beta;
    }
    DevIn<SpatialDescJob> dj(jobs);
    launch_spatial_desc(nullptr, dj.p, (int)jobs.size(), max_nb, dtb->b(), kListener);
    sync_check();
    const std::vector<uint8_t> got = dtb->host_bytes(tb0.size());
    std::vector<char> is_loose(tb0.size(), 0);
    auto looser = [&](float g, float w, int kind, bool exact, const char* what, size_t where) {
      if (kind == 0) {
        const uint32_t u = ulp_distance(g, w);
        t.w_ulp = std::max(t.w_ulp, u);
        if (u > 1 && !t.w++) t.first += fmt(" first w: %s %zu got %.9g want %.9g", what, where, (double)g, (double)w);
        return;
      }
      const double rel = g == w ? 0.0 : std::fabs((double)g - (double)w) / std::max(std::fabs((double)w), 1e-30);
      t.gain_rel = std::max(t.gain_rel, rel == rel ? rel : 1e300);
      t.gain_bits += bits(g) != bits(w);
      if ((exact ? bits(g) != bits(w) : !(rel <= 1e-6)) && !t.gain++) t.first += fmt(" first gain: %s %zu got %.9g want %.9g", what, where, (double)g, (double)w);
    };
    for (const Loose& l : loose) {
      for (int i = 0; i < 4; i++) is_loose[l.off + (size_t)i] = 1;
      float g, w;
      std::memcpy(&g, got.data() + l.off, 4);
      std::memcpy(&w, want.data() + l.off, 4);
      looser(g, w, l.kind, l.exact, "table byte", l.off);
    }
    // every other byte: idx, the fade bit, seg and the other flag bits, the EQ table, entry 0, and what no job names
    for (size_t j = 0; j < specs.size(); j++) {
      const DSpec& s = specs[j];
      for (int b = 0; b <= s.nblocks; b++) {
        const size_t off = desc_off[j] + (size_t)b * sizeof(SpatialDesc);
        sr::Desc g, w;
        std::memcpy(&g, got.data() + off, sizeof g);
        std::memcpy(&w, want.data() + off, sizeof w);
        const bool mine = b >= s.b0 + 1 && b <= s.b0 + s.nb;
        size_t bad = 0;
        if (mine) {
          for (int q = 0; q < 4; q++) bad += g.idx[q] != w.idx[q];
          if (bad && !t.idx) t.first += fmt(" first idx: job %zu block %d got %d %d %d %d want %d %d %d %d", j, b - 1, g.idx[0], g.idx[1], g.idx[2], g.idx[3], w.idx[0], w.idx[1], w.idx[2], w.idx[3]);
          t.idx += bad;
          if ((g.flags & 1) != (w.flags & 1) && !t.fade++) t.first += fmt(" first fade bit: job %zu block %d got %d want %d", j, b - 1, g.flags & 1, w.flags & 1);
          t.host_fields += g.seg != w.seg || (g.flags & ~1) != (w.flags & ~1);
        } else if (b == 0) {
          t.entry0 += std::memcmp(&g, &w, sizeof g) != 0;
        }
        for (size_t i = 0; i < sizeof(SpatialEqEntry); i++) t.eq += got[eq_off[j] + (size_t)b * sizeof(SpatialEqEntry) + i] != want[eq_off[j] + (size_t)b * sizeof(SpatialEqEntry) + i];
      }
    }
    for (size_t i = 0; i < got.size(); i++) t.stray += !is_loose[i] && got[i] != want[i];
    // (a byte counted above as idx, fade bit, seg, EQ or entry 0 is counted here again: any of them fails the check)
    const std::vector<uint8_t> cb = dcarry->host_bytes(specs.size() * 2 * sizeof(SpatialCarry));
    for (size_t j = 0; j < specs.size(); j++) {
      SpatialCarry g;
      std::memcpy(&g, cb.data() + (j * 2 + 1) * sizeof g, sizeof g);
      const SpatialCarry& w = wcarry[j];
      size_t bad = 0;
      for (int q = 0; q < 4; q++) {
        bad += g.idx[q] != w.idx[q];
        looser(g.w[q], w.w[q], 0, false, "carried record of job", j);
      }
      looser(g.g, w.g, 1, specs[j].exact_gain, "carried g of job", j);
      bad += bits(g.beta) != bits(w.beta) || (uint32_t)g.pad_[0] != kCD || (uint32_t)g.pad_[1] != kCD;
      SpatialCarry in;   // prev_in is read, never written
      std::memcpy(&in, cb.data() + j * 2 * sizeof in, sizeof in);
      SpatialCarry in0;
      std::memset(&in0, 0xCD, sizeof in0);
      if (specs[j].prev == kPrevIn) std::memcpy(&in0, &specs[j].carry, 40);
      bad += std::memcmp(&in, &in0, sizeof in) != 0;
      t.carry += bad;
    }
    t.guards += dtb->guard_damage() + dcarry->guard_damage();
    for (const auto& m : dmod) t.guards += m->guard_damage();
  }
  SpatialCarry carried_out(size_t j) const {
    const std::vector<uint8_t> cb = dcarry->host_bytes(specs.size() * 2 * sizeof(SpatialCarry));
    SpatialCarry g;
    std::memcpy(&g, cb.data() + (j * 2 + 1) * sizeof g, sizeof g);
    g.pad_[0] = g.pad_[1] = 0;
    return g;
  }
};
static void desc_case(const std::string& name, const std::vector<DSpec>& specs, int want_fades = -1) {
  DescRig rig(specs);
  DescTally t;
  rig.run(t);
  bool ok = t.ok();
  if (want_fades == 0) ok = ok && t.fades_seen == 0 && t.steady_seen > 0;   // identical consecutive parameter vectors must not fade
  if (want_fades > 0) ok = ok && t.fades_seen >= (size_t)want_fades;        // vectors that differ in one parameter must
  check(name, ok, "%s", t.str().c_str());
}
static std::vector<float> ramp(int n, float a, float step, int hold) {   // a, a, ..(hold times), a + step, ...: consecutive blocks equal inside a hold
  std::vector<float> v((size_t)n);
  for (int i = 0; i < n; i++) v[(size_t)i] = a + step * (float)(i / hold);
  return v;
}
static void family_desc() {
  uint64_t seed = 0xDE5C0000u;
  // every parameter from `value`: nb = 1, 63, 64, 65 (one and two workgroups of lanes), b0 > 0; nothing fades behind block b0
  for (int nb : {1, 63, 64, 65}) {
    sr::Rng rng{seed++};
    DSpec s;
    desc_defaults(s, rng);
    s.nblocks = nb + 3;
    s.b0 = nb == 1 ? 0 : 2;
    s.nb = nb;
    s.flags0 = nb % 2 ? 3 : 0;
    desc_case(fmt("desc.value.nb%d", nb), {s}, nb > 1 ? 0 : -1);
  }
  // from curve_off: the position moves every second block (one parameter differs: a fade; equal vectors: none); linear model
  {
    sr::Rng rng{seed++};
    DSpec s;
    desc_defaults(s, rng);
    s.nblocks = s.nb = 65;
    s.model = kSpatialLinear;
    s.value[7] = 40.f;
    s.curve[0] = ramp(65, 0.83f, 0.0625f, 2);
    s.curve[2] = ramp(65, -2.41f, 0.f, 1);
    desc_case("desc.curve.nb65", {s}, 32);
  }
  // from mod: sample 0 of the block, clamped at vmin in some blocks and at vmax in others; a curve under one modulation input
  {
    sr::Rng rng{seed++};
    DSpec s;
    desc_defaults(s, rng);
    s.nblocks = 12;
    s.b0 = 1;
    s.nb = 10;
    s.vmin[0] = -1.5f;
    s.vmax[0] = 2.25f;
    s.value[0] = 0.4f;
    s.mod[0] = {0.f, -3.f, -0.7f, 0.3f, 5.f, 1.1f, -9.f, 0.9f, 2.f, 1.85f, 1.85f, 0.f};   // below vmin in blocks 1 and 6, above vmax in 4 and 8
    s.curve[1] = ramp(12, -0.6f, 0.11f, 1);
    s.mod[1] = std::vector<float>(12, 0.05f);
    s.mod[12] = ramp(12, -0.5f, 0.03125f, 3);   // spatialBlend 0.75 + mod, clamped to [0, 1]
    s.vmin[12] = 0.f;
    s.vmax[12] = 1.f;
    desc_case("desc.mod", {s}, 5);
  }
  // two jobs of different nb in one launch (lanes of the second workgroup of lanes have nothing to do in the first job)
  {
    sr::Rng rng{seed++};
    DSpec a, b;
    desc_defaults(a, rng);
    desc_defaults(b, rng);
    a.nblocks = 6;
    a.b0 = 1;
    a.nb = 5;
    a.A = 4;
    a.D = 12;
    a.curve[2] = ramp(6, -1.3f, -0.21f, 1);
    b.nblocks = b.nb = 70;
    b.model = kSpatialLinear;
    b.value[7] = 25.f;
    b.curve[0] = ramp(70, -3.1f, 0.09f, 1);
    b.flags0 = 2;
    desc_case("desc.two_jobs", {a, b}, 60);
  }
  // a cone and the exponential model: acos and pow are rounded once from double on the device too, but through the device's
  // libraries: 1e-6 relative, the bound tests/test_gpu_spatial.py holds the device's gain to
  for (int model : {kSpatialInverse, kSpatialExponential}) {
    sr::Rng rng{seed++};
    DSpec s;
    desc_defaults(s, rng);
    s.nblocks = s.nb = 9;
    s.model = model;
    s.exact_gain = false;
    s.value[3] = -0.3f;
    s.value[4] = 0.1f;
    s.value[5] = 0.9f;
    s.value[9] = 40.f;
    s.value[10] = 300.f;
    s.value[11] = 0.25f;
    s.value[8] = 1.3f;
    s.curve[0] = ramp(9, -2.2f, 0.55f, 1);
    desc_case(model == kSpatialInverse ? "desc.cone" : "desc.cone_exponential", {s}, 6);
  }
  // occlusion: the EQ table is written and the largest band factor joins g (float32 operations: bit for bit)
  {
    sr::Rng rng{seed++};
    DSpec s;
    desc_defaults(s, rng);
    s.nblocks = 8;
    s.b0 = 1;
    s.nb = 6;
    s.occlusion = true;
    s.curve[13] = {0.f, 0.f, 0.f, 0.3f, 0.3f, 1.f, 0.65f, 0.f};
    s.value[14] = 0.9f;
    s.value[15] = 0.4f;
    s.value[16] = 0.1f;
    desc_case("desc.eq", {s}, 3);
  }
  // the carried descriptor: none; from the host (a record that differs: block b0 fades); on the device with b0 = 0 (entry 0 is
  // written, idx clamped to the set: the record's idx lies outside it) and with b0 > 0 (entry 0 is left alone)
  {
    sr::Rng rng{seed++};
    DSpec s;
    desc_defaults(s, rng);
    s.nblocks = 5;
    s.nb = 3;
    SpatialCarry c{};
    c.idx[0] = 3;
    c.idx[1] = 44;
    c.idx[2] = -2;
    c.idx[3] = 39;
    c.w[0] = 0.5f;
    c.w[1] = 0.25f;
    c.w[2] = 0.125f;
    c.w[3] = 0.125f;
    c.g = 0.7f;
    c.beta = 0.3f;
    DSpec none = s, host = s, in0 = s, in2 = s;
    host.prev = kPrevHost;
    host.carry = c;
    in0.prev = kPrevIn;
    in0.carry = c;
    in2.prev = kPrevIn;
    in2.carry = c;
    in2.b0 = 2;
    desc_case("desc.prev.none", {none}, 0);
    desc_case("desc.prev.host", {host}, 1);
    desc_case("desc.prev.in_b0", {in0}, 1);
    desc_case("desc.prev.in_b2", {in2}, 1);
    // what one launch left in prev_out, handed to the next as prev_in and as prev_host with the same parameters: no fade
    DescRig first({none});
    DescTally t0;
    first.run(t0);
    DSpec chain_in = s, chain_host = s;
    chain_in.prev = kPrevIn;
    chain_host.prev = kPrevHost;
    chain_in.carry = chain_host.carry = first.carried_out(0);
    chain_in.b0 = chain_host.b0 = 2;
    desc_case("desc.prev.chain", {chain_in, chain_host}, 0);
  }
}

// =====================================================================================================================
//  head
// =====================================================================================================================
static void family_head() {
  const double kRate[4] = {48000.0, 44100.0, 48000.0, 44100.0}, kRadius[4] = {0.0875, 0.0875, 0.07, 0.11};
  int c = 0;
  for (int taps : {1, 63, 64, 65, 512})
    for (int gap : {0, 3}) {
      const double fs = kRate[c % 4], a = kRadius[c % 4];
      c++;
      const int64_t stride = taps + gap;
      const int channels = 2 * kSpatialHeadDirs;
      Guarded out((size_t)channels * (size_t)stride * 4);
      launch_spatial_head(nullptr, out.f(), stride, taps, fs, a);
      sync_check();
      const std::vector<float> got = out.host((size_t)channels * (size_t)stride);
      std::vector<float> want((size_t)channels * (size_t)taps);
      parallel_for((size_t)channels, [&](size_t ch) {
        const SpatialHeadEar e = spatial_head_ear(fs, a, (int)ch);
        for (int k = 0; k < taps; k++) want[ch * (size_t)taps + (size_t)k] = spatial_head_tap(e, k);
      });
      size_t wrong = 0, stray = 0, not_bits = 0;
      double worst = 0.0, peak = 0.0;
      std::string first;
      for (size_t ch = 0; ch < (size_t)channels; ch++)
        for (int64_t k = 0; k < stride; k++) {
          const float g = got[ch * (size_t)stride + (size_t)k];
          if (k >= taps) {
            stray += !is_cd(g);
            continue;
          }
          const float w = want[ch * (size_t)taps + (size_t)k], aw = std::fabs(w);
          const double lim = std::max((double)(std::nextafterf(aw, INFINITY) - aw), std::ldexp(1.0, -40)), err = std::fabs((double)g - (double)w);
          peak = std::max(peak, (double)aw);
          not_bits += bits(g) != bits(w);
          worst = std::max(worst, err == err ? err / lim : 1e300);
          if (!(err <= lim) && !wrong++) first = fmt(" first: channel %zu tap %lld got %.9g want %.9g", ch, (long long)k, (double)g, (double)w);
        }
      const size_t guards = out.guard_damage();
      // (tap 0 of every channel is zero -- the delay is at least the kernel's half-width -- so taps = 1 is a set of zeros)
      check(fmt("head.t%d.s%d", taps, gap), !wrong && !stray && !guards && (peak > 0.0 || taps == 1),
            "fs %.0f a %.4f: taps %zu beyond max(1 ulp, 2^-40) %zu (largest ratio %.3f, not the host's bits %zu, peak %.3f), gap not 0xCD %zu, guards %zu%s", fs, a, want.size(), wrong, worst,
            not_bits, peak, stray, guards, first.c_str());
    }
}

int main(int argc, char** argv) {
  const std::string fam = argc > 1 ? argv[1] : "";
  const auto t0 = std::chrono::steady_clock::now();
  if (fam != "panner" && fam != "float" && fam != "direct" && fam != "desc" && fam != "head") {
    std::printf("usage: spatial_kernels_check panner|float|direct|desc|head\n");
    return 2;
  }
  CK(hipFree(nullptr));
  if (fam == "panner") family_panner();
  else if (fam == "float") family_float();
  else if (fam == "direct") family_direct();
  else if (fam == "desc") family_desc();
  else family_head();
  std::printf("time %s %.2f s\n", fam.c_str(), std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  if (failures) std::printf("%d checks failed\n", failures);
  return failures ? 1 : 0;
}
