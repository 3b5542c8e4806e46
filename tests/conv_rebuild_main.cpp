// Stand-alone host check of the convolver migration's index arithmetic (graphaudio_amd/csrc/ga_conv_rebuild.hpp; option "conv_migrate").
// The rebuild kernel's loops are replayed on the host over arrays of exactly the sizes the planner allocates (D's input history of
// coarseP x 8192 samples per channel, the node's [bInCh][129][P-1] stores, the scratch planes [rows][129][tx]); every element carries
// a tag (channel, bin, block), so a wrong offset shows as a wrong tag or a missing element, and an offset outside an array is the
// address sanitizer's (tests/test_conv_migrate_host.py builds this file with -fsanitize=address,undefined).  The same program checks
// the set builder that the private-IR convolver stage and the migration share (conv_for_each_set).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ga_conv_rebuild.hpp"

using namespace ga;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { failures++; std::printf("FAIL %s:%d ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static float tag(int ch, int k, int j) { return (float)(((ch * 200 + k) * 2048 + j) + 1); }

struct Node { int P, bInCh, bSlots; bool shared, trueStereo; };

// what conv_rebuild_kernel does for one job, with the sample reads reduced to their addresses
static void rebuild_job(const ConvRebuildJob& J, int ch, std::vector<float>& planeR, int tx, int hist, std::vector<double>& sampleSum) {
  const int FB_RUN = 32;
  for (int t0 = 0; t0 < (J.P + FB_RUN - 1) / FB_RUN * FB_RUN; t0 += FB_RUN) {
    if (t0 >= J.P) continue;
    for (int wave = 0; wave < 4; wave++)
      for (int q = 0; q < FB_RUN / 4; q++) {
        const int t = t0 + wave + 4 * q;
        if (!J.src || t >= J.P) continue;
        for (int lane = 0; lane < 64; lane++) {
          const float* p = J.src + (int64_t)t * kRebuildBlock + 2 * lane;
          sampleSum[t] += (double)p[0] + (double)p[1];
        }
      }
    for (int idx = 0; idx < kRebuildBins * FB_RUN; idx++) {
      const int k = idx >> 5, q = idx & (FB_RUN - 1), j = t0 + q;
      if (j >= J.P) continue;
      planeR[conv_rebuild_plane_index(J.xrow, tx, hist, J.P, k, j)] = tag(ch, k, j);
      if (j >= 1) J.dst_r[conv_rebuild_store_index(J.P, k, j)] = tag(ch, k, j);
    }
  }
}

static void run(const std::vector<Node>& nodes) {
  int maxP = 1;
  for (const Node& n : nodes) maxP = n.P > maxP ? n.P : maxP;
  const int hist = conv_rebuild_hist(maxP), tx = conv_rebuild_tx(maxP);
  CHECK(hist % 4 == 0 && hist >= maxP - 1 && tx == hist + 4, "plane geometry for P = %d", maxP);
  struct State { std::vector<std::vector<float>> hist; std::vector<float> store; int x0; };
  std::vector<State> st(nodes.size());
  std::vector<ConvRebuildJob> jobs;
  std::vector<int> jobNode, jobCh;
  for (size_t i = 0; i < nodes.size(); i++) {
    const Node& n = nodes[i];
    const int64_t hl = ((int64_t)n.P * kRebuildBlock + 8191) / 8192 * 8192;   // coarseP x 8192
    st[i].store.assign((size_t)n.bInCh * kRebuildBins * (n.P - 1 > 1 ? n.P - 1 : 1), 0.f);
    st[i].x0 = (int)jobs.size();
    const int nxr = n.shared ? 1 : n.bInCh;
    for (int ch = 0; ch < nxr; ch++) {
      st[i].hist.emplace_back((size_t)hl);
      for (int64_t s = 0; s < hl; s++) st[i].hist[ch][s] = (float)(s - (hl - (int64_t)n.P * kRebuildBlock));   // sample index relative to block T-P
    }
    for (int ch = 0; ch < nxr; ch++) {
      const size_t hstride = (size_t)kRebuildBins * (n.P - 1 > 1 ? n.P - 1 : 1);
      jobs.push_back(ConvRebuildJob{st[i].hist[ch].data() + conv_rebuild_src_offset(hl, n.P), st[i].store.data() + ch * hstride, nullptr, n.P,
                                    (int)jobs.size()});
      jobNode.push_back((int)i);
      jobCh.push_back(ch);
    }
  }
  std::vector<float> planeR(jobs.size() * kRebuildBins * (size_t)tx, 0.f);
  for (size_t j = 0; j < jobs.size(); j++) {
    const Node& n = nodes[jobNode[j]];
    std::vector<double> sums(n.P, 0.0);
    rebuild_job(jobs[j], jobCh[j], planeR, tx, hist, sums);
    // block t of the job is samples [128 t, 128 t + 128) counted from block T-P: the last block ends at the history's last sample
    for (int t = 0; t < n.P; t++) {
      const double want = 128.0 * (128.0 * t) + 127.0 * 128.0 / 2.0;
      CHECK(sums[t] == want, "P %d block %d reads the wrong samples (%f, expected %f)", n.P, t, sums[t], want);
    }
  }
  for (size_t i = 0; i < nodes.size(); i++) {
    const Node& n = nodes[i];
    const int h = n.P - 1, nxr = n.shared ? 1 : n.bInCh;
    const size_t hstride = (size_t)kRebuildBins * (h > 1 ? h : 1);
    for (int ch = 0; ch < n.bInCh; ch++)
      for (int k = 0; k < kRebuildBins; k++)
        for (int c = 0; c < h; c++) {   // [ch][k][c] <-> block T-P+1+c ; channels beyond a shared node's first stay zero
          const float want = ch < nxr ? tag(ch, k, c + 1) : 0.f;
          CHECK(st[i].store[ch * hstride + (size_t)k * h + c] == want, "store of node %zu: [%d][%d][%d]", i, ch, k, c);
        }
    for (int ch = 0; ch < nxr; ch++)
      for (int k = 0; k < kRebuildBins; k++)
        for (int col = 0; col < tx; col++) {   // the partition sum of block T-1 reads column hist - p for partition p
          const int j = col - (hist - (n.P - 1));
          const float want = (j >= 0 && j < n.P) ? tag(ch, k, j) : 0.f;
          CHECK(planeR[((size_t)(st[i].x0 + ch) * kRebuildBins + k) * tx + col] == want, "plane of node %zu: row %d bin %d column %d", i, ch, k, col);
        }
    // every slot finds its input channel's row, in both slot layouts
    int seen = 0;
    for (int xc = 0; xc < nxr; xc++)
      for (int slot = 0; slot < n.bSlots; slot++)
        if (n.shared || conv_slot_input(n.trueStereo, slot) == xc) seen++;
    CHECK(seen == n.bSlots, "node %zu: %d of %d slots have an x row", i, seen, n.bSlots);
    if (n.trueStereo) CHECK(conv_slot_input(true, 0) == 0 && conv_slot_input(true, 1) == 0 && conv_slot_input(true, 2) == 1 && conv_slot_input(true, 3) == 1, "true stereo slots");
  }
  std::printf("checked %zu nodes, %zu jobs, planes %d columns\n", nodes.size(), jobs.size(), tx);
}

// conv_for_each_set: the planner's sets of one node.  Every slot exactly once, no run longer than a set, a run's x-row is the input
// channel of each of its slots (0 when the node's one row is shared), runs in increasing x-row, then increasing slot.
static void check_sets(bool shared, bool trueStereo, int bInCh, int bSlots) {
  const int nxr = shared ? 1 : bInCh;
  std::vector<int> emitted(bSlots, 0);
  int runs = 0, lastXc = -1, lastSlot = -1;
  conv_for_each_set(shared, trueStereo, nxr, bSlots, [&](int xc, const int* slots, int ncol) {
    runs++;
    CHECK(ncol >= 1 && ncol <= kConvSetCols && kConvSetCols == 16, "run of %d slots", ncol);
    CHECK(xc >= 0 && xc < nxr && xc >= lastXc, "x-row %d after %d of %d", xc, lastXc, nxr);
    if (xc != lastXc) lastSlot = -1;
    lastXc = xc;
    for (int j = 0; j < ncol; j++) {
      const int slot = slots[j];
      CHECK(slot >= 0 && slot < bSlots, "slot %d of %d", slot, bSlots);
      if (slot < 0 || slot >= bSlots) continue;
      emitted[slot]++;
      CHECK(slot > lastSlot, "slot %d after %d on x-row %d", slot, lastSlot, xc);
      lastSlot = slot;
      CHECK(xc == (shared ? 0 : conv_slot_input(trueStereo, slot)), "slot %d on x-row %d", slot, xc);
    }
  });
  for (int slot = 0; slot < bSlots; slot++)
    CHECK(emitted[slot] == 1, "shared %d true stereo %d, %d slots: slot %d emitted %d times", (int)shared, (int)trueStereo, bSlots, slot, emitted[slot]);
  // as few runs as the rule allows: a shared row is cut every 16 slots, a row of its own holds the slots that read it (1, or 2 in true stereo)
  const int want = shared ? (bSlots + kConvSetCols - 1) / kConvSetCols : nxr;
  CHECK(runs == want, "shared %d true stereo %d, %d slots: %d runs, expected %d", (int)shared, (int)trueStereo, bSlots, runs, want);
}

int main() {
  for (int shared = 0; shared < 2; shared++) {
    check_sets(shared != 0, true, 2, 4);
    for (int ch = 1; ch <= 33; ch++) check_sets(shared != 0, false, ch, ch);
  }
  std::printf("checked the sets of %d slot layouts\n", 2 * 34);
  for (int P : {1, 2, 71, 1101}) {
    run({Node{P, 1, 1, true, false}});
    run({Node{P, 2, 2, true, false}});     // a mono signal in both channels of a two-channel response: one row
    run({Node{P, 2, 2, false, false}});
    run({Node{P, 2, 4, false, true}});     // true stereo (L,h0)(L,h1)(R,h2)(R,h3)
    run({Node{P, 2, 4, true, true}});
  }
  // nodes of different lengths in one launch: the shorter ones' blocks end at the same column
  run({Node{71, 2, 2, false, false}, Node{1, 1, 1, true, false}, Node{1101, 2, 4, false, true}, Node{2, 2, 2, true, false}});
  std::printf(failures ? "failures %d\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
