// tests/spatial_ref.hpp against itself: built with g++ under the address and undefined-behaviour sanitizers and run directly (no GPU, no
// HIP) by tests/test_spatial_ref_host.py.  argv[1] is tests/golden/spatial_ref_case.bin.  One line per check,
// "check <name> ok|FAIL <figures>"; exit status 1 if any check fails.
//   a_vs_naive         form (a) against a double loop over sum_k F[k] m[n - k] written on its own here (its own mix, taps, fade), 1e-12
//                      of sum |F||m| + |dry x|; mono, stereo, silent blocks, fades, T = 1, 2, 129, 512
//   a_vs_model         form (a) against tests/_spatial_model.render on the recorded case (tests/golden/make_spatial_ref_case.py), 1e-12
//   b_within_bound     form (b) within gamma_c (sum |F||m| + |dry x|) of form (a), c = T + 9 (tests/spatial_kernels_main.hip derives it)
//   b_exact            on the exact scenes form (b) IS form (a): every written sample and the history, bit for bit
//   chunk_cut_a / _b   nine blocks cut at every block, the history handed on: the same bits as one piece, in both forms
//   works              plan_works / span_works cover every processed block once, one work carries the history, panner_facts holds; a
//                      table with a block in two works, a fade behind silence or an idx outside the set is refused
//   direct_walk_cut    the occlusion walk over 9 blocks against 4 + 5 with the state handed on: the same bits, the same state
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "spatial_ref.hpp"

namespace sr = spatial_ref;

static int failures = 0;
static void check(const char* name, bool ok, double figure, const char* what) {
  std::printf("check %s %s %s %.3e\n", name, ok ? "ok" : "FAIL", what, figure);
  if (!ok) failures++;
}

// the naive statement: nothing shared with render64 but the tables
static double naive_ratio(const sr::Node& nd, const sr::Rendered<double>& got) {
  const int T = nd.taps;
  double worst = 0.0;
  auto m = [&](int64_t f) -> double {
    if (f < -512) return 0.0;
    if (f < 0) return nd.hist_in[512 + f];
    const sr::Desc& d = nd.desc[f / 128 + 1];
    if (d.seg < 0) return 0.0;
    const double l = nd.segs[d.seg].in_l[f];
    return (d.flags & 2) ? (l + (double)nd.segs[d.seg].in_r[f]) / 2.0 : l;
  };
  for (int64_t b = 0; b < nd.nblocks; b++) {
    const sr::Desc& d = nd.desc[b + 1];
    if ((d.seg >= 0) != (got.written[(size_t)b] != 0)) return 1e300;
    if (d.seg < 0) continue;
    for (int e = 0; e < 2; e++)
      for (int n = 0; n < 128; n++) {
        const int64_t f = b * 128 + n;
        const double x = (e == 1 && (d.flags & 2)) ? nd.segs[d.seg].in_r[f] : nd.segs[d.seg].in_l[f];
        double y[2] = {0.0, 0.0}, mag[2] = {0.0, 0.0};
        for (int v = 0; v < ((d.flags & 1) ? 2 : 1); v++) {
          const sr::Desc& dd = nd.desc[b + 1 - v];
          for (int k = 0; k < T; k++) {
            double F = 0.0;
            for (int q = 0; q < 4; q++) F += (double)dd.w[q] * nd.hrir[(2 * dd.idx[q] + e) * nd.hstride + k];
            F *= dd.gb;
            y[v] += F * m(f - k);
            mag[v] += std::fabs(F * m(f - k));
          }
          y[v] += (double)dd.dry * x;
          mag[v] += std::fabs((double)dd.dry * x);
        }
        double want = y[0], mg = mag[0];
        if (d.flags & 1) {
          const double w = (n + 1) / 128.0;
          want = w * y[0] + (1.0 - w) * y[1];
          mg = w * mag[0] + (1.0 - w) * mag[1];
        }
        const double err = std::fabs(got.out[e][(size_t)f] - want);
        if (err > 0.0) worst = std::max(worst, err / mg);
        if (std::fabs(got.mag[e][(size_t)f] - mg) > 1e-12 * mg) return 1e300;
      }
  }
  for (int i = 0; i < 512; i++)
    if (got.hist[(size_t)i] != m(nd.nblocks * 128 - 512 + i)) return 1e300;
  return worst;
}

static double bits_differ(const sr::Rendered<double>& a, const sr::Rendered<float>& b) {
  double bad = 0;
  for (int e = 0; e < 2; e++)
    for (size_t f = 0; f < a.out[e].size(); f++)
      if (a.written[f / 128] && (double)b.out[e][f] != a.out[e][f]) bad++;
  for (size_t i = 0; i < 512; i++) bad += (double)b.hist[i] != a.hist[i];
  return bad;
}

int main(int argc, char** argv) {
  sr::Rng rng{20261021};
  const char* const kPatterns[] = {"m", "s", "mss-m", "-mm-m-ss-", "ssmm--"};
  {
    double worst = 0.0;
    for (int T : {1, 2, 129, 512})
      for (const char* pat : kPatterns)
        for (int fade = 0; fade < 3; fade++) {
          const sr::HrirSet set = sr::make_hrir(rng, 5, T, T + (fade == 1 ? 3 : 0), false);
          sr::NodeScene S;
          sr::make_node(S, rng, set, pat, (sr::Fade)fade, false, fade != 0, fade == 2);
          worst = std::max(worst, naive_ratio(S.node(), sr::render64(S.node())));
        }
    check("a_vs_naive", worst <= 1e-12, worst, "max |a - naive| / (sum |F||m| + |dry x|)");
  }
  {
    double worst = 1e300;
    FILE* f = argc > 1 ? std::fopen(argv[1], "rb") : nullptr;
    int h[5] = {0, 0, 0, 0, 0};
    if (f && std::fread(h, 4, 5, f) == 5 && h[0] == 0x31415053 && h[4] == 1) {
      const int T = h[1], D = h[2], nb = h[3];
      const size_t N = (size_t)nb * 128;
      std::vector<float> hrir((size_t)(D * 2 * T)), x(2 * N), hist(512);
      std::vector<sr::Desc> desc((size_t)nb + 1);
      std::vector<double> want(2 * N);
      static_assert(sizeof(sr::Desc) == 48, "the recorded descriptors are 48 bytes");
      if (std::fread(hrir.data(), 4, hrir.size(), f) == hrir.size() && std::fread(x.data(), 4, x.size(), f) == x.size() &&
          std::fread(hist.data(), 4, 512, f) == 512 && std::fread(desc.data(), sizeof(sr::Desc), desc.size(), f) == desc.size() &&
          std::fread(want.data(), 8, want.size(), f) == want.size()) {
        const sr::Seg seg{x.data(), x.data() + N};
        const sr::Node nd{hrir.data(), T, T, desc.data(), &seg, 1, hist.data(), nb, D};
        const sr::Rendered<double> got = sr::render64(nd);
        worst = 0.0;
        int silent = 0;
        for (int e = 0; e < 2; e++)
          for (size_t i = 0; i < N; i++) {
            if (!got.written[i / 128]) {
              silent++;
              if (want[e * N + i] != 0.0) worst = 1e300;
              continue;
            }
            worst = std::max(worst, std::fabs(got.out[e][i] - want[e * N + i]) / got.mag[e][i]);
          }
        if (silent != 256 || sr::panner_facts(&nd, 1, sr::plan_works(desc.data(), nb, 0).data(), (int)sr::plan_works(desc.data(), nb, 0).size())) worst = 1e300;
      }
    }
    if (f) std::fclose(f);
    check("a_vs_model", worst <= 1e-12, worst, "max |a - model| / (sum |F||m| + |dry x|)");
  }
  {
    double worst = 0.0;
    const double u = std::ldexp(1.0, -24);
    for (int T : {1, 3, 129, 512})
      for (const char* pat : kPatterns)
        for (int fade = 0; fade < 2; fade++) {
          const sr::HrirSet set = sr::make_hrir(rng, 5, T, T, false);
          sr::NodeScene S;
          sr::make_node(S, rng, set, pat, (sr::Fade)fade, false, true, false);
          const sr::Rendered<double> a = sr::render64(S.node());
          const sr::Rendered<float> b = sr::render32(S.node());
          const double c = T + 9, gamma = c * u / (1.0 - c * u);
          for (int e = 0; e < 2; e++)
            for (size_t f = 0; f < a.out[e].size(); f++)
              if (a.written[f / 128]) worst = std::max(worst, std::fabs((double)b.out[e][f] - a.out[e][f]) / (gamma * a.mag[e][f]));
          if (a.written != b.written) worst = 1e300;
        }
    check("b_within_bound", worst <= 1.0, worst, "max |b - a| / (gamma_c (sum |F||m| + |dry x|))");
  }
  {
    double bad = 0;
    for (int T : {1, 2, 3, 127, 128, 129, 511, 512})
      for (const char* pat : kPatterns) {
        const sr::HrirSet set = sr::make_hrir(rng, 6, T, T + 1, true);
        sr::NodeScene S;
        sr::make_node(S, rng, set, pat, sr::kFadeEvery, true, true, true);
        bad += bits_differ(sr::render64(S.node()), sr::render32(S.node()));
      }
    check("b_exact", bad == 0, bad, "samples of form (b) that are not form (a)'s value on the exact scenes");
  }
  for (int form = 0; form < 2; form++) {
    double bad = 0;
    for (int T : {2, 129, 512}) {
      // inputs of 12 bits: the stereo mix is a float32, so form (a)'s history passes through hist_in unrounded
      const sr::HrirSet set = sr::make_hrir(rng, 5, T, T, false);
      sr::NodeScene S;
      sr::make_node(S, rng, set, "mmss-smm-", sr::kFadeEvery, false, true, false);
      for (float& v : S.in) v = v == v ? std::ldexp(std::floor(std::ldexp(v, 11)), -11) : v;
      for (float& v : S.hist) v = std::ldexp(std::floor(std::ldexp(v, 11)), -11);
      const sr::Rendered<double> a1 = sr::render64(S.node());
      const sr::Rendered<float> b1 = sr::render32(S.node());
      for (int cut = 1; cut < 9; cut++) {
        std::vector<sr::Seg> segs;
        std::vector<float> hist = S.hist;
        for (int piece = 0; piece < 2; piece++) {
          const int64_t g0 = piece ? cut : 0, len = piece ? 9 - cut : cut;
          const sr::Node nd = sr::slice_node(S, g0, len, hist.data(), segs);
          std::vector<float> next(512);
          if (form == 0) {
            const sr::Rendered<double> p = sr::render64(nd);
            for (int e = 0; e < 2; e++)
              for (size_t f = 0; f < p.out[e].size(); f++) bad += p.written[f / 128] != a1.written[(size_t)g0 + f / 128] || p.out[e][f] != a1.out[e][(size_t)g0 * 128 + f];
            for (int i = 0; i < 512; i++) bad += (double)(next[(size_t)i] = (float)p.hist[(size_t)i]) != p.hist[(size_t)i];
            if (piece)
              for (int i = 0; i < 512; i++) bad += p.hist[(size_t)i] != a1.hist[(size_t)i];
          } else {
            const sr::Rendered<float> p = sr::render32(nd);
            for (int e = 0; e < 2; e++)
              for (size_t f = 0; f < p.out[e].size(); f++) bad += p.written[f / 128] != b1.written[(size_t)g0 + f / 128] || p.out[e][f] != b1.out[e][(size_t)g0 * 128 + f];
            next = p.hist;
            if (piece)
              for (int i = 0; i < 512; i++) bad += p.hist[(size_t)i] != b1.hist[(size_t)i];
          }
          hist = next;
        }
      }
    }
    check(form ? "chunk_cut_b" : "chunk_cut_a", bad == 0, bad, "samples that differ between one piece and two");
  }
  {
    double bad = 0;
    for (const char* pat : {"m", "mmmm", "mmmmm", "mss-m", "-mm-m-ss-", "ssmm--", "---", "mmmmmmmmm"}) {
      const sr::HrirSet set = sr::make_hrir(rng, 3, 4, 4, true);
      sr::NodeScene S;
      sr::make_node(S, rng, set, pat, sr::kFadeEvery, true, false, false);
      const sr::Node nd = S.node();
      if (std::string(pat) == "---") {   // (nblocks >= 1 and no processed block: the history alone)
        const std::vector<sr::Work> w = sr::plan_works(S.desc.data(), S.n, 0);
        bad += !(w.size() == 1 && w[0].nb == 0 && w[0].b0 == 3 && w[0].tail == 1);
      }
      for (int mode = 0; mode < 2; mode++) {
        std::vector<sr::Work> w = mode ? sr::span_works(S.n, 0) : sr::plan_works(S.desc.data(), S.n, 0);
        bad += sr::panner_facts(&nd, 1, w.data(), (int)w.size()) != nullptr;
        w.push_back(w[0]);
        bad += (w[0].nb > 0 || w[0].tail) && sr::panner_facts(&nd, 1, w.data(), (int)w.size()) == nullptr;
      }
    }
    const sr::HrirSet set = sr::make_hrir(rng, 3, 4, 4, true);
    sr::NodeScene S;
    sr::make_node(S, rng, set, "m-m", sr::kFadeNone, true, false, false);
    const sr::Node nd = S.node();
    const std::vector<sr::Work> w = sr::plan_works(S.desc.data(), S.n, 0);
    S.desc[3].flags |= 1;
    bad += sr::panner_facts(&nd, 1, w.data(), (int)w.size()) == nullptr;
    S.desc[3].flags &= ~1;
    S.desc[1].idx[2] = 3;
    bad += sr::panner_facts(&nd, 1, w.data(), (int)w.size()) == nullptr;
    check("works", bad == 0, bad, "tables judged wrongly");
  }
  {
    double bad = 0;
    const ga::SpatialBands K = ga::spatial_bands(48000.0);
    const ga::SpatialEq I{1.0f, 0.0f, 0.0f}, Q{0.5f, 0.25f, -0.125f}, R{0.75f, 0.f, 0.25f};
    // identity, a run that the cut at 4 opens, identity, a second run from zero state
    const std::vector<ga::SpatialEq> eqs = {I, I, Q, R, R, Q, I, I, R, I};   // entry 0 is not used
    std::vector<float> x(2 * 9 * 128), one(x.size(), -7.f), two(x.size(), -7.f);
    for (float& v : x) v = rng.unit();
    for (int stereo = 0; stereo < 2; stereo++) {
      sr::DirectJob j{{x.data(), stereo ? x.data() + 9 * 128 : nullptr}, {one.data(), stereo ? one.data() + 9 * 128 : nullptr}, eqs.data(), I, 0, 0, 0, 0, 9};
      sr::DirectState s1{}, s2{};
      sr::direct_walk(K, j, s1);
      j.out[0] = two.data();
      j.out[1] = stereo ? two.data() + 9 * 128 : nullptr;
      j.nb = 4;
      sr::direct_walk(K, j, s2);
      bad += s2.open[0] != 1 || s2.open[1] != stereo;
      j.b0 = 4;
      j.nb = 5;
      j.from_state = 1;
      j.prev_valid = 1;
      sr::direct_walk(K, j, s2);
      bad += std::memcmp(&s1, &s2, sizeof s1) != 0 || s1.open[0] != 1;
      for (size_t i = 0; i < (size_t)(stereo ? 2 : 1) * 9 * 128; i++) bad += std::memcmp(&one[i], &two[i], 4) != 0;
      for (int i = 0; i < 128; i++) bad += one[(size_t)i] != x[(size_t)i] || one[(size_t)(6 * 128 + i)] != x[(size_t)(6 * 128 + i)];   // identity blocks are copies
    }
    check("direct_walk_cut", bad == 0, bad, "samples or state fields that differ between 9 blocks and 4 + 5");
  }
  if (failures) std::printf("%d checks failed\n", failures);
  return failures ? 1 : 0;
}
