// tests/spatial_ref.hpp -- the contracts of the SpatialPannerNode kernels (graphaudio_amd/csrc/ga_spatial.hip) as plain C++, written
// from ga_kernels.hpp ("SpatialPannerNode ...", SpatialDesc / SpatialSeg / SpatialJob / SpatialWork, SpatialDescJob, SpatialDirectJob)
// and DESIGN.md section 2e, not from the kernels.  No HIP headers: tests/spatial_ref_main.cpp builds it with g++ under the
// sanitizers (tests/test_spatial_ref_host.py), tests/spatial_kernels_main.hip holds the kernels to it (tests/test_gpu_spatial_kernels.py).
// Build with -ffp-contract=off: form (b) is float32 operation for operation.
//
// The panner, per node and chunk of `nblocks` blocks of 128 frames (table entry b + 1 = block b, entry 0 = the block in front):
//   m[f]      the mono mix: in_l[f], or 0.5 (in_l[f] + in_r[f]) for a stereo block (flags bit 1); 0 in a silent block (seg < 0);
//             hist_in[512 + f] for -512 <= f < 0; 0 in front of that
//   F_b[e][k] = gb_b * sum_{q < 4} w_b[q] hrir[(2 idx_b[q] + e) hstride + k],   k < T
//   y_b[e][n] = sum_{k < T} F_b[e][k] m[128 b + n - k] + dry_b x_e[128 b + n]       (x_1 = x_0 for a mono block)
//   out       = y_b, or, where flags bit 0 of entry b + 1 is set, w_n y_b + (1 - w_n) y_{b-1 -> b}, w_n = (n + 1) / 128, with
//             y_{b-1 -> b} the same sums over block b's frames with entry b's filters and dry gain.  Silent blocks are not written.
//   hist_out  the last 512 samples of [hist_in | m]
// in two forms: (a) float64 throughout (Render64), (b) the float32 chain the header promises (Render32): a tap is four fmaf in
// ascending q from 0, then gb *; a sum is fmaf(F[k], m[n - k], acc) in ascending k from 0; the output is fmaf(dry, x, sum); the fade
// is fmaf(w_n, y, (1 - w_n) * fmaf(dry', x, sum')).
// Occlusion and geometry are ga_spatial_direct.hpp and ga_spatial_geom.hpp themselves (both build with a plain host compiler); here
// is the walk over blocks around them: have, open, runs of active blocks, the carried state.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "ga_spatial_direct.hpp"
#include "ga_spatial_geom.hpp"

namespace spatial_ref {

constexpr int kBlock = 128, kMaxTaps = 512, kRun = 4;

struct Desc {   // = ga::SpatialDesc
  int idx[4];
  float w[4];
  float gb, dry;
  int seg, flags;
};
struct Seg {    // = ga::SpatialSeg, host pointers, chunk-frame indexed
  const float* in_l;
  const float* in_r;
};
struct Work {   // = ga::SpatialWork
  int job, b0, nb, tail;
};
struct Node {   // = ga::SpatialJob with its tables, host pointers
  const float* hrir;
  int64_t hstride;
  int taps;
  const Desc* desc;      // [nblocks + 1]
  const Seg* segs;
  int nsegs;
  const float* hist_in;  // [512]
  int64_t nblocks;
  int dirs;              // directions of the set (what idx is checked against)
};

inline double mix64(const Node& nd, int64_t f) {
  if (f < 0) return f >= -(int64_t)kMaxTaps ? (double)nd.hist_in[kMaxTaps + f] : 0.0;
  const Desc& d = nd.desc[1 + f / kBlock];
  if (d.seg < 0) return 0.0;
  const Seg& s = nd.segs[d.seg];
  return (d.flags & 2) ? 0.5 * ((double)s.in_l[f] + (double)s.in_r[f]) : (double)s.in_l[f];
}
inline float mix32(const Node& nd, int64_t f) {
  if (f < 0) return f >= -(int64_t)kMaxTaps ? nd.hist_in[kMaxTaps + f] : 0.f;
  const Desc& d = nd.desc[1 + f / kBlock];
  if (d.seg < 0) return 0.f;
  const Seg& s = nd.segs[d.seg];
  return (d.flags & 2) ? 0.5f * (s.in_l[f] + s.in_r[f]) : s.in_l[f];
}
inline double tap64(const Node& nd, const Desc& d, int ear, int k) {
  double a = 0.0;
  for (int q = 0; q < 4; q++) a += (double)d.w[q] * (double)nd.hrir[(int64_t)(2 * d.idx[q] + ear) * nd.hstride + k];
  return (double)d.gb * a;
}
inline float tap32(const Node& nd, const Desc& d, int ear, int k) {
  float a = 0.f;
  for (int q = 0; q < 4; q++) a = fmaf(d.w[q], nd.hrir[(int64_t)(2 * d.idx[q] + ear) * nd.hstride + k], a);
  return d.gb * a;
}

template <class R>
struct Rendered {
  std::vector<R> out[2];        // [nblocks * 128], untouched where written is 0
  std::vector<char> written;    // per block
  std::vector<R> hist;          // [512]
  std::vector<double> mag[2];   // form (a) only: w_n (sum |F||m| + |dry x|) + (1 - w_n) (the same of the previous filters)
};

// form (a)
inline Rendered<double> render64(const Node& nd) {
  const int T = nd.taps;
  const int64_t n = nd.nblocks, N = n * kBlock;
  Rendered<double> o;
  for (int e = 0; e < 2; e++) {
    o.out[e].assign((size_t)N, 0.0);
    o.mag[e].assign((size_t)N, 0.0);
  }
  o.written.assign((size_t)n, 0);
  std::vector<double> m((size_t)(N + kMaxTaps));   // m[kMaxTaps + f]
  for (int64_t f = -kMaxTaps; f < N; f++) m[(size_t)(kMaxTaps + f)] = mix64(nd, f);
  o.hist.assign(m.end() - kMaxTaps, m.end());
  std::vector<double> F[2][2];   // [cur | prev][ear]
  for (int64_t b = 0; b < n; b++) {
    const Desc& d = nd.desc[b + 1];
    if (d.seg < 0) continue;
    const Desc& p = nd.desc[b];
    const bool fade = (d.flags & 1) != 0, stereo = (d.flags & 2) != 0;
    for (int e = 0; e < 2; e++) {
      F[0][e].resize((size_t)T);
      F[1][e].assign((size_t)T, 0.0);
      for (int k = 0; k < T; k++) {
        F[0][e][(size_t)k] = tap64(nd, d, e, k);
        if (fade) F[1][e][(size_t)k] = tap64(nd, p, e, k);
      }
    }
    const Seg& s = nd.segs[d.seg];
    o.written[(size_t)b] = 1;
    for (int i = 0; i < kBlock; i++) {
      const int64_t f = b * kBlock + i;
      const double wn = (double)(i + 1) / (double)kBlock;
      for (int e = 0; e < 2; e++) {
        const double x = (double)((e && stereo) ? s.in_r[f] : s.in_l[f]);
        double yc = 0.0, yp = 0.0, mc = 0.0, mp = 0.0;
        for (int k = 0; k < T; k++) {
          const double mk = m[(size_t)(kMaxTaps + f - k)];
          yc += F[0][e][(size_t)k] * mk;
          mc += std::fabs(F[0][e][(size_t)k] * mk);
          yp += F[1][e][(size_t)k] * mk;
          mp += std::fabs(F[1][e][(size_t)k] * mk);
        }
        yc += (double)d.dry * x;
        mc += std::fabs((double)d.dry * x);
        if (fade) {
          yp += (double)p.dry * x;
          mp += std::fabs((double)p.dry * x);
          yc = wn * yc + (1.0 - wn) * yp;
          mc = wn * mc + (1.0 - wn) * mp;
        }
        o.out[e][(size_t)f] = yc;
        o.mag[e][(size_t)f] = mc;
      }
    }
  }
  return o;
}

// form (b)
inline Rendered<float> render32(const Node& nd) {
  const int T = nd.taps;
  const int64_t n = nd.nblocks, N = n * kBlock;
  Rendered<float> o;
  for (int e = 0; e < 2; e++) o.out[e].assign((size_t)N, 0.f);
  o.written.assign((size_t)n, 0);
  std::vector<float> m((size_t)(N + kMaxTaps));
  for (int64_t f = -kMaxTaps; f < N; f++) m[(size_t)(kMaxTaps + f)] = mix32(nd, f);
  o.hist.assign(m.end() - kMaxTaps, m.end());
  std::vector<float> F[2][2];
  for (int64_t b = 0; b < n; b++) {
    const Desc& d = nd.desc[b + 1];
    if (d.seg < 0) continue;
    const Desc& p = nd.desc[b];
    const bool fade = (d.flags & 1) != 0, stereo = (d.flags & 2) != 0;
    for (int e = 0; e < 2; e++) {
      F[0][e].resize((size_t)T);
      F[1][e].assign((size_t)T, 0.f);
      for (int k = 0; k < T; k++) {
        F[0][e][(size_t)k] = tap32(nd, d, e, k);
        if (fade) F[1][e][(size_t)k] = tap32(nd, p, e, k);
      }
    }
    const Seg& s = nd.segs[d.seg];
    o.written[(size_t)b] = 1;
    for (int i = 0; i < kBlock; i++) {
      const int64_t f = b * kBlock + i;
      for (int e = 0; e < 2; e++) {
        const float x = (e && stereo) ? s.in_r[f] : s.in_l[f];
        float yc = 0.f, yp = 0.f;
        for (int k = 0; k < T; k++) {
          const float mk = m[(size_t)(kMaxTaps + f - k)];
          yc = fmaf(F[0][e][(size_t)k], mk, yc);
          if (fade) yp = fmaf(F[1][e][(size_t)k], mk, yp);
        }
        float y = fmaf(d.dry, x, yc);
        if (fade) {
          const float wn = (float)(i + 1) * (1.0f / kBlock);
          y = fmaf(wn, y, (1.0f - wn) * fmaf(p.dry, x, yp));
        }
        o.out[e][(size_t)f] = y;
      }
    }
  }
  return o;
}

// the workgroups of a node as Context::planSpatialPanner cuts them: every segment (a run of blocks of one seg >= 0) in runs of up to
// kRun blocks, the run that ends the chunk carries the history; a chunk that ends on silence gets a work of no blocks for it
inline std::vector<Work> plan_works(const Desc* desc, int64_t n, int job) {
  std::vector<Work> w;
  bool tailDone = false;
  for (int64_t b = 0; b < n;) {
    const int sg = desc[b + 1].seg;
    int64_t e = b + 1;
    while (e < n && desc[e + 1].seg == sg) e++;
    if (sg >= 0)
      for (int64_t b0 = b; b0 < e; b0 += kRun) {
        const int nb = (int)std::min<int64_t>(kRun, e - b0);
        const bool tail = b0 + nb == n;
        tailDone = tailDone || tail;
        w.push_back(Work{job, (int)b0, nb, tail ? 1 : 0});
      }
    b = e;
  }
  if (!tailDone) w.push_back(Work{job, (int)n, 0, 1});
  return w;
}
// the same chunk in runs of kRun blocks whatever their segments: silent blocks fall inside the runs
inline std::vector<Work> span_works(int64_t n, int job) {
  std::vector<Work> w;
  for (int64_t b0 = 0; b0 < n; b0 += kRun) {
    const int nb = (int)std::min<int64_t>(kRun, n - b0);
    w.push_back(Work{job, (int)b0, nb, b0 + nb == n ? 1 : 0});
  }
  return w;
}

// the contract of the tables (ga_kernels.hpp): null when it holds, else what does not
inline const char* panner_facts(const Node* nodes, int nnodes, const Work* works, int nworks) {
  std::vector<std::vector<int>> cover((size_t)nnodes);
  std::vector<int> tails((size_t)nnodes, 0);
  for (int j = 0; j < nnodes; j++) {
    const Node& nd = nodes[j];
    if (nd.taps < 1 || nd.taps > kMaxTaps || nd.hstride < nd.taps || nd.nblocks < 1 || nd.dirs < 1) return "taps, hstride, nblocks or dirs";
    cover[(size_t)j].assign((size_t)nd.nblocks, 0);
    for (int64_t b = 0; b <= nd.nblocks; b++) {
      const Desc& d = nd.desc[b];
      for (int q = 0; q < 4; q++)
        if (d.idx[q] < 0 || d.idx[q] >= nd.dirs) return "idx outside the set";
      if (b == 0) continue;
      if (d.seg >= nd.nsegs) return "seg outside the table";
      if (d.seg < 0) continue;
      if (!nd.segs[d.seg].in_l || ((d.flags & 2) && !nd.segs[d.seg].in_r)) return "a segment's view is null";
      if ((d.flags & 1) && b > 1 && nd.desc[b - 1].seg < 0) return "a block behind a silent block fades";
    }
  }
  for (int i = 0; i < nworks; i++) {
    const Work& w = works[i];
    if (w.job < 0 || w.job >= nnodes) return "work.job";
    const Node& nd = nodes[w.job];
    if (w.nb < 0 || w.nb > kRun || w.b0 < 0 || w.b0 + w.nb > nd.nblocks) return "work.b0 / nb";
    for (int b = w.b0; b < w.b0 + w.nb; b++)
      if (cover[(size_t)w.job][(size_t)b]++) return "a block belongs to two works";
    if (w.tail) tails[(size_t)w.job]++;
  }
  for (int j = 0; j < nnodes; j++) {
    if (tails[(size_t)j] != 1) return "not exactly one work writes the history";
    for (int64_t b = 0; b < nodes[j].nblocks; b++)
      if (nodes[j].desc[b + 1].seg >= 0 && !cover[(size_t)j][(size_t)b]) return "a processed block belongs to no work";
  }
  return nullptr;
}

// ---- occlusion / transmission: one node over blocks [b0, b0 + nb), both channels, as ga_kernels.hpp states SpatialDirectJob ------------
struct DirectState {   // = ga::SpatialDirectState
  float zl[2], zh[2];
  ga::SpatialEq prev;
  int open[2];
};
struct DirectJob {
  const float* in[2];          // chunk-frame indexed; in[1] null: mono
  float* out[2];
  const ga::SpatialEq* eqs;    // eqs[b + 1] = block b
  ga::SpatialEq prev;
  int open, from_state, prev_valid, b0, nb;
};
// The first processed block after creation or silence (prev_valid 0) ramps from its own triple.  A block is active when its own or the
// previous triple is not the identity; the filters run in active blocks only, from zero state where the run is not open; other
// blocks are copied.  The state keeps zl / zh, whether the last block was active (per channel held) and the last triple.
inline void direct_walk(const ga::SpatialBands& K, const DirectJob& j, DirectState& st) {
  const DirectState in = st;
  for (int ch = 0; ch < 2; ch++) {
    const bool walks = j.in[ch] != nullptr;
    float zl = 0.f, zh = 0.f;
    ga::SpatialEq pr{1.0f, 0.0f, 0.0f};
    bool have = false, open = false;
    if (walks) {
      have = j.prev_valid != 0;
      pr = j.from_state ? in.prev : j.prev;
      open = (j.from_state ? in.open[ch] != 0 : ((j.open >> ch) & 1) != 0) && have;
      if (open) {
        zl = in.zl[ch];
        zh = in.zh[ch];
      }
      for (int b = j.b0; b < j.b0 + j.nb; b++) {
        const ga::SpatialEq cur = j.eqs[b + 1];
        if (!have) pr = cur;
        const bool active = !ga::spatial_eq_identity(cur) || !ga::spatial_eq_identity(pr);
        const float* x = j.in[ch] + (int64_t)b * kBlock;
        float* y = j.out[ch] + (int64_t)b * kBlock;
        if (active) {
          if (!open) zl = zh = 0.f;
          for (int n = 0; n < kBlock; n++) y[n] = ga::spatial_direct_step(K, ga::spatial_eq_at(pr, cur, n), x[n], zl, zh);
        } else {
          for (int n = 0; n < kBlock; n++) y[n] = x[n];
        }
        open = active;
        have = true;
        pr = cur;
      }
    }
    st.zl[ch] = zl;
    st.zh[ch] = zh;
    st.open[ch] = (walks && open) ? 1 : 0;
    if (ch == 0) st.prev = pr;
  }
}

// ---- descriptors of signal-driven nodes: one block's parameter vector -> geometry, EQ triple, descriptor ---------------------------
// the k-rate value (AudioParam.ComputeKRate): the intrinsic value, plus sample 0 of the modulation input and the clamp where there is one
inline float krate(float intrinsic, const float* mod0, float vmin, float vmax) {   // mod0: sample 0 of the block's modulation input, null: silent
  return mod0 ? ga::spatial_clamp(intrinsic + *mod0, vmin, vmax) : intrinsic;
}
inline void desc_block(const float* pv, const float* L, int model, int A, int D, bool occlusion, ga::SpatialGeom& g, ga::SpatialEq& eq) {
  ga::spatial_geometry<ga::SpatialMathDouble>(pv, L, model, A, D, g);
  eq = ga::SpatialEq{1.0f, 0.0f, 0.0f};
  if (occlusion) {
    float s;
    ga::spatial_occlusion(pv[13], pv[14], pv[15], pv[16], s, eq);
    g.g = g.g * s;
  }
}
inline void desc_fill(const ga::SpatialGeom& g, int D, Desc& d) {   // seg and flags are not touched
  for (int q = 0; q < 4; q++) {
    d.idx[q] = std::min(std::max(g.idx[q], 0), std::max(D, 1) - 1);
    d.w[q] = g.w[q];
  }
  d.gb = g.g * g.beta;
  d.dry = g.g * (1.0f - g.beta);
}
// how far a block is from the definition's jumps: pa and pe from an integer, the directivity from 0.999, and the distance.  The
// direction is the geometry's own float32 statements; everything behind it is double.
struct DescMargins {
  double pa, pe, directivity, distance;
};
inline DescMargins desc_margins(const float* pv, const float* L, int A, int D) {
  DescMargins mg{1.0, 1.0, 1.0, 0.0};
  float wx = pv[0] - L[0], wy = pv[1] - L[1], wz = pv[2] - L[2];
  const float distance = std::sqrt(wx * wx + wy * wy + wz * wz);
  mg.distance = distance;
  if (!(distance > 0.0001f)) return mg;
  const float inv = 1.0f / distance;
  wx *= inv;
  wy *= inv;
  wz *= inv;
  const float dx = wx * L[3] + wy * L[4] + wz * L[5], dy = wx * L[6] + wy * L[7] + wz * L[8], dz = wx * L[9] + wy * L[10] + wz * L[11];
  const double PI = 3.14159265358979323846;
  double az = std::atan2((double)dx, -(double)dz) * (180.0 / PI);
  if (az < 0.0) az += 360.0;
  const double pa = az * (double)A / 360.0;
  mg.pa = std::fabs(pa - std::round(pa));
  const int E = D / A;
  if (E > 1) {
    const double y = dy < -1.f ? -1.0 : (dy > 1.f ? 1.0 : (double)dy);
    const double pe = (std::asin(y) * (180.0 / PI) + 90.0) / 180.0 * (double)(E - 1);
    mg.pe = std::fabs(pe - std::round(pe));
  }
  if (pv[9] < 360.f || pv[10] < 360.f) {
    const double om = std::sqrt((double)pv[3] * pv[3] + (double)pv[4] * pv[4] + (double)pv[5] * pv[5]);
    if (om > 0.0001) {
      double dot = -((double)pv[3] * wx + (double)pv[4] * wy + (double)pv[5] * wz) / om;
      dot = dot < -1.0 ? -1.0 : (dot > 1.0 ? 1.0 : dot);
      const double ang = std::acos(dot) * 180.0 / PI, hi = 0.5 * pv[9], ho = 0.5 * pv[10];
      double dir = 1.0;
      if (ang <= hi) dir = 1.0;
      else if (ang >= ho) dir = pv[11];
      else dir = 1.0 + (ang - hi) / (ho - hi) * ((double)pv[11] - 1.0);
      mg.directivity = std::fabs(dir - 0.999);
    }
  }
  return mg;
}
inline bool desc_margins_ok(const DescMargins& m) { return m.pa >= 1e-6 && m.pe >= 1e-6 && m.directivity >= 1e-4 && m.distance >= 0.01; }


// ---- test scenes: one node with its HRIR set, descriptors, segments and input rows, drawn from a seed -------------------------------
// (shared by tests/spatial_ref_main.cpp and tests/spatial_kernels_main.hip, so that the host checks and the device checks see the
// same kind of data).  exact: x integers in [-3, 3], taps integers in [-2, 2], w one of (1,0,0,0), (1/2,1/2,0,0), (1/2,0,1/2,0),
// (1/4,1/4,1/4,1/4), gb 1/2, 1 or 2, dry 0, 1/2 or 1 -- every float32 operation of form (b) is then exact, in any order.
// Otherwise x uniform in [-1, 1), bilinear weights, gb in [1/4, 1], dry in [0, 1); the taps are uniform in [-1, 1) with the sign
// of tap k of an ear shared by all directions, so that the four taps that meet in one filter tap do not cancel and |F_k| is the
// magnitude its five roundings are relative to.
struct Rng {   // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  float unit() { return (float)((double)(int64_t)(next() >> 40) / 8388608.0 - 1.0); }   // 24 bits -> [-1, 1), exact
  int below(int n) { return (int)(next() % (uint64_t)n); }
};
struct HrirSet {
  int dirs, taps;
  int64_t hstride;
  std::vector<float> h;   // [2 dirs][hstride], NaN behind tap `taps` of a channel
};
inline HrirSet make_hrir(Rng& rng, int dirs, int T, int64_t hstride, bool exact) {
  HrirSet S{dirs, T, hstride, std::vector<float>((size_t)(2 * dirs * hstride), std::nanf(""))};
  std::vector<float> sign((size_t)(2 * T));
  for (float& v : sign) v = rng.below(2) ? 1.f : -1.f;
  for (int c = 0; c < 2 * dirs; c++)
    for (int k = 0; k < T; k++)
      S.h[(size_t)(c * hstride + k)] = exact ? (float)(rng.below(5) - 2) : sign[(size_t)((c & 1) * T + k)] * std::fabs(rng.unit());
  return S;
}
enum Fade { kFadeNone = 0, kFadeEvery = 1, kFadeFirst = 2 };
struct NodeScene {
  const HrirSet* set = nullptr;
  int64_t n = 0;
  std::vector<Desc> desc;          // [n + 1]; entry 0 is a descriptor of its own, seg -1
  std::vector<float> in;           // the segments' rows; NaN wherever the contract reads nothing
  std::vector<int64_t> off_l, off_r;   // per segment: where chunk frame 0 of the view lies in `in` (off_r -1: mono)
  std::vector<float> hist;         // [512]
  std::vector<Seg> segs;
  Node node() const { return Node{set->h.data(), set->hstride, set->taps, desc.data(), segs.data(), (int)segs.size(), hist.data(), n, set->dirs}; }
};
inline void draw_desc(Rng& rng, int dirs, bool exact, Desc& d) {
  static const float kW[4][4] = {{1.f, 0.f, 0.f, 0.f}, {.5f, .5f, 0.f, 0.f}, {.5f, 0.f, .5f, 0.f}, {.25f, .25f, .25f, .25f}};
  static const float kGb[3] = {.5f, 1.f, 2.f}, kDry[3] = {0.f, .5f, 1.f};
  for (int q = 0; q < 4; q++) d.idx[q] = rng.below(dirs);
  if (exact) {
    const int p = rng.below(4);
    for (int q = 0; q < 4; q++) d.w[q] = kW[p][q];
    d.gb = kGb[rng.below(3)];
    d.dry = kDry[rng.below(3)];
  } else {
    const double fa = 0.5 * (rng.unit() + 1.0), fe = 0.5 * (rng.unit() + 1.0);
    d.w[0] = (float)((1.0 - fe) * (1.0 - fa));
    d.w[1] = (float)((1.0 - fe) * fa);
    d.w[2] = (float)(fe * (1.0 - fa));
    d.w[3] = (float)(fe * fa);
    d.gb = 0.625f + 0.375f * rng.unit();
    d.dry = 0.5f * (rng.unit() + 1.0f);
  }
}
// pattern: one letter per block, 'm' mono, 's' stereo, '-' silent; a segment is a run of equal letters
inline void make_node(NodeScene& S, Rng& rng, const HrirSet& set, const char* pattern, Fade fade, bool exact, bool hist_nonzero, bool offset_views) {
  S.set = &set;
  int64_t n = 0;
  while (pattern[n]) n++;
  S.n = n;
  const int64_t N = n * kBlock, row = (N + 4 + 3) / 4 * 4;
  S.desc.assign((size_t)(n + 1), Desc{});
  auto value = [&]() { return exact ? (float)(rng.below(7) - 3) : rng.unit(); };
  S.hist.assign((size_t)kMaxTaps, 0.f);
  if (hist_nonzero)
    for (float& v : S.hist) v = exact ? 0.5f * (float)(rng.below(13) - 6) : rng.unit();
  draw_desc(rng, set.dirs, exact, S.desc[0]);
  S.desc[0].seg = -1;
  int last = -1;
  for (int64_t b = 0; b < n; b++) {
    Desc& d = S.desc[(size_t)(b + 1)];
    draw_desc(rng, set.dirs, exact, d);
    const char c = pattern[b];
    if (c == '-') {
      d.seg = -1;
      continue;
    }
    last = (int)b;
    const bool stereo = c == 's';
    if (b == 0 || pattern[b - 1] != c) {   // a new segment: its rows
      for (int ch = 0; ch < (stereo ? 2 : 1); ch++) {
        const int64_t base = (int64_t)S.in.size() + (offset_views ? 1 + ch : 0);
        S.in.resize(S.in.size() + (size_t)row, std::nanf(""));
        (ch ? S.off_r : S.off_l).push_back(base);
      }
      if (!stereo) S.off_r.push_back(-1);
    }
    d.seg = (int)S.off_l.size() - 1;
    for (int i = 0; i < kBlock; i++) {
      S.in[(size_t)(S.off_l.back() + b * kBlock + i)] = value();
      if (stereo) S.in[(size_t)(S.off_r.back() + b * kBlock + i)] = value();
    }
    const bool prevProcessed = b == 0 || pattern[b - 1] != '-';
    const bool f = prevProcessed && (fade == kFadeEvery || (fade == kFadeFirst && b == 0));
    d.flags = (f ? 1 : 0) | (stereo ? 2 : 0);
  }
  if (last >= 0) S.desc[(size_t)(last + 1)].idx[3] = set.dirs - 1;   // the set's last direction is reached
  S.desc[0].idx[0] = set.dirs - 1;
  S.segs.clear();
  for (size_t s = 0; s < S.off_l.size(); s++) S.segs.push_back(Seg{S.in.data() + S.off_l[s], S.off_r[s] < 0 ? nullptr : S.in.data() + S.off_r[s]});
}
// blocks [g0, g0 + len) of a node as a chunk of their own: entry 0 is the table's entry g0, the views are moved by g0 blocks
inline Node slice_node(const NodeScene& S, int64_t g0, int64_t len, const float* hist, std::vector<Seg>& segs) {
  segs.clear();
  for (const Seg& s : S.segs) segs.push_back(Seg{s.in_l + g0 * kBlock, s.in_r ? s.in_r + g0 * kBlock : nullptr});
  Node nd = S.node();
  nd.desc = S.desc.data() + g0;
  nd.segs = segs.data();
  nd.hist_in = hist;
  nd.nblocks = len;
  return nd;
}

}  // namespace spatial_ref
