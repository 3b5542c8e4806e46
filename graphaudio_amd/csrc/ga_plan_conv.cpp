// ga_plan_conv.cpp -- the convolver stages of a chunk: formulation D (coarse partitions, fused groups, pre-mix, carried tails), the shared-IR
// groups of formulation A, formulations B / C / R on private state, scratch sizing (see ga_chunk_internal.hpp).
#include "ga_chunk_internal.hpp"

namespace ga {

// ======================================================================================================
// convolver rows <-> groups
// ======================================================================================================
// make sure the group's state arrays cover all rows; new rows start from zero state
void Context::ensureGroupState(ConvGroup& g) {
  Context& c = *this;
  int need = (int)roundup(std::max<size_t>(g.rows.size(), 1), 128);
  if (need <= g.rp) return;
  const int hist = g.P - 1;
  size_t hBytes = (size_t)kBins * std::max(hist, 1) * need * sizeof(float);
  size_t oBytes = (size_t)need * kBlock * sizeof(float);
  float* nr = (float*)c.dalloc(hBytes);
  float* ni = (float*)c.dalloc(hBytes);
  float* o0 = (float*)c.dalloc(oBytes);
  float* o1 = (float*)c.dalloc(oBytes);
  GA_HIP(hipMemsetAsync(nr, 0, hBytes, c.stream));
  GA_HIP(hipMemsetAsync(ni, 0, hBytes, c.stream));
  GA_HIP(hipMemsetAsync(o0, 0, oBytes, c.stream));
  GA_HIP(hipMemsetAsync(o1, 0, oBytes, c.stream));
  if (g.rp > 0) {
    if (hist > 0 && !g.histZero) {
      GA_HIP(hipMemcpy2DAsync(nr, (size_t)need * 4, g.histR, (size_t)g.rp * 4, (size_t)g.rp * 4, (size_t)kBins * hist,
                              hipMemcpyDeviceToDevice, c.stream));
      GA_HIP(hipMemcpy2DAsync(ni, (size_t)need * 4, g.histI, (size_t)g.rp * 4, (size_t)g.rp * 4, (size_t)kBins * hist,
                              hipMemcpyDeviceToDevice, c.stream));
    }
    GA_HIP(hipMemcpyAsync(o0, g.overlap[g.ovCur], (size_t)g.rp * kBlock * 4, hipMemcpyDeviceToDevice, c.stream));
    c.syncStream();
    size_t oldH = (size_t)kBins * std::max(hist, 1) * g.rp * sizeof(float);
    c.dfree(g.histR, oldH);
    c.dfree(g.histI, oldH);
    c.dfree(g.overlap[0], (size_t)g.rp * kBlock * 4);
    c.dfree(g.overlap[1], (size_t)g.rp * kBlock * 4);
  }
  g.histR = nr;
  g.histI = ni;
  g.overlap[0] = o0;
  g.overlap[1] = o1;
  g.ovCur = 0;
  g.rp = need;
}

// ======================================================================================================
// formulation D (ga_coarse.hip): coarse partitions, consumer sums fused in the frequency domain
// ======================================================================================================
// Which convolver outputs may be summed as spectra?  A node whose single output feeds exactly ONE input (or parameter) of
// one consumer, and is a term of that input in every segment of the chunk.  Every mixing rule of AudioNodeInput.MixBuffer
// (equal counts, 1 -> N, N -> 1 down-mix, min(N, M), AudioNodeInput.cs:182-244) is linear in the term, so the consumer
// may receive the sum of the group as ONE term -- the leader's output -- and nothing from the other members.  What changes
// is only the association of the float32 additions (the reference adds the members one by one in connection order).
void Context::planCoarseFusion(const std::vector<int>& topo, const std::vector<Segment>& segs) {
  // The grouping is a function of the graph, of the convolvers' formulations and impulse responses and of the segments' control
  // state (who is a term of which input): while none of them moved since the previous chunk the leaders stand.
  {
    uint64_t key = hmix(graphVersion, (uint64_t)segs.size());
    for (const Segment& sg : segs) key = hmix(key, sg.hash);
    for (int id : topo) {
      if (nodes[id]->type != GA_NODE_CONVOLVER) continue;
      const ConvolverS& nd = rec<ConvolverS>(*nodes[id]);
      key = hmix(hmix(key, ((uint64_t)id << 8) | (uint64_t)nd.convPath), (uint64_t)(uintptr_t)nd.ir.get());
    }
    if (fusionKeyValid && key == fusionKey) return;
    fusionKey = key;
    fusionKeyValid = true;
  }
  std::vector<int> cand;
  for (int id : topo) {
    if (nodes[id]->type != GA_NODE_CONVOLVER) continue;
    ConvolverS& nd = rec<ConvolverS>(*nodes[id]);
    nd.dLeader = -1;
    if (!nd.ir || nd.convPath != 4) continue;
    nd.dLeader = id;
    if (nd.outputs[0].connectedInputs.size() == 1) cand.push_back(id);
  }
  if (cand.size() < 2) return;
  std::unordered_map<int, int> seen;                 // candidate -> segments in which it is a term of its consumer's input
  std::unordered_map<int, std::vector<int>> byConsumer;
  for (int id : cand) {
    seen[id] = 0;
    byConsumer[nodes[id]->outputs[0].connectedInputs[0].node].push_back(id);
  }
  for (const Segment& sg : segs)
    for (const NodeSeg& ns : sg.nodes) {
      if (byConsumer.find(ns.id) == byConsumer.end()) continue;
      auto scan = [&](const InSeg& is, int inputIdx) {
        for (const TermS& t : is.terms) {
          auto it = seen.find(t.node);
          if (it == seen.end()) continue;
          const InRef& r = nodes[t.node]->outputs[0].connectedInputs[0];
          if (r.node == ns.id && r.input == inputIdx && t.out == 0) it->second++;
        }
      };
      for (int i = 0; i < (int)ns.ins.size(); i++) scan(ns.ins[i], i);
      for (int p = 0; p < (int)ns.pins.size(); p++) scan(ns.pins[p], -1 - p);
    }
  std::map<std::tuple<int, int, int, int, int>, int> leaderOf;   // (consumer, input, depth, output channels, partitions) -> leader
  for (int id : cand) {   // topo order: the leader is the first member the traversal reaches
    ConvolverS& nd = rec<ConvolverS>(*nodes[id]);
    if (seen[id] != (int)segs.size()) continue;
    const InRef& r = nd.outputs[0].connectedInputs[0];
    auto key = std::make_tuple(r.node, r.input, nd.depth, nd.effectiveOutCh, nd.ir->coarseP);
    auto it = leaderOf.find(key);
    if (it == leaderOf.end()) leaderOf.emplace(key, id);
    else nd.dLeader = it->second;
  }
}

// chunk-long view of input channel `c` of a convolver: the segment views when they agree, else a materialised copy
static const float* convChunkInput(Context& c, Exec& ex, const Exec::ConvInRow& ci, int ch) {
  const auto& segs = ex.segs;
  const float* stable = nullptr;
  bool same = true, first = true;
  for (size_t si = 0; si < segs.size(); si++) {
    const float* v = (ci[si].empty() || ch >= (int)ci[si].size()) ? nullptr : ci[si][ch];
    if (first) { stable = v; first = false; } else if (v != stable) same = false;
  }
  if (same) return stable;
  float* slab = getSlab(c);
  for (size_t si = 0; si < segs.size(); si++) {
    const float* v = (ci[si].empty() || ch >= (int)ci[si].size()) ? nullptr : ci[si][ch];
    MixJob mj;
    mj.out = slab;
    mj.term0 = (int)ex.terms.size();
    mj.nterms = v ? 1 : 0;
    mj.f0 = segs[si].b0 * kBlock;
    mj.n = (segs[si].b1 - segs[si].b0) * kBlock;
    if (v) {
      ex.terms.push_back(v);
      ex.noteAlign(v, mj.f0);
    }
    ex.mixJobs.push_back(mj);
  }
  return slab;
}

// true stereo: the slab that slot `slot` of node `id` renders into; chunkPlanConvolvers sums the four of a node into its two outputs
static float* trueStereoTemp(Context& c, ConvPlanCtx& k, int id, int slot) {
  float* tmp = getSlab(c);
  k.tsTemps.emplace(id, std::array<float*, 4>{}).first->second[slot] = tmp;
  return tmp;
}

// one set of the B / R partition sums: x-row `x`, y rows from `y0`, the spectra of the slots' impulse-response channels (slot index ==
// IR channel index in both slot layouts)
static ConvSetB makeSetB(const IrSpectra& ir, int x, int y0, const int* slots, int ncol) {
  ConvSetB st{};
  st.x = x;
  st.y0 = y0;
  st.ncol = ncol;
  st.P = ir.P;
  for (int j = 0; j < ncol; j++) {
    st.hr[j] = ir.hr + (size_t)slots[j] * kBins * ir.P;
    st.hi[j] = ir.hi + (size_t)slots[j] * kBins * ir.P;
  }
  return st;
}

// the hist_len samples in front of the chunk of input channel `ch`: a span of a PlayableAudioBuffer, the node's own copy, or nothing yet
static const float* coarseHistory(const ConvolverS& nd, int ch) {
  if (ch < (int)nd.dHistExt.size() && nd.dHistExt[ch].first) return nd.dHistExt[ch].first;
  return nd.dHistZero ? nullptr : nd.dHist[nd.dHistCur] + (size_t)ch * nd.dHistLen;
}

// If the last hist_len samples of this chunk's input are device memory that stays (a PlayableAudioBuffer played zero-copy), the
// next chunk's history is that span and nothing has to be written; otherwise the span is forgotten and the caller copies.
static bool coarseHistoryStays(Context& c, ConvolverS& nd, int ch, const float* in, int64_t frames) {
  if ((int)nd.dHistExt.size() < nd.bInCh) nd.dHistExt.resize(nd.bInCh, {nullptr, -1});
  const int64_t hl = nd.dHistLen;
  int buf = -1;
  if (c.coarseExtHist && in && frames >= hl) buf = c.persistentBuffer(in + (frames - hl), hl);
  nd.dHistExt[ch] = buf >= 0 ? std::make_pair(in + (frames - hl), buf) : std::make_pair((const float*)nullptr, -1);
  return buf >= 0;
}

// One convolver stage of a chunk in formulation D, planned in five passes (Context::chunkPlanConvolvers calls planCoarseStage).
namespace {
struct CoarseStage {
  Context& c;
  Exec& ex;
  const std::vector<int>& dNodes;
  const int64_t n, frames;
  const int nT;
  static constexpr int kVoicesPerJob = kCoarseJobTerms;   // terms whose products one workgroup accumulates in registers
  struct Piece {   // <= 4 columns of one signal: (impulse-response channel, output channel of the group)
    int frame0, P, xrow, u0;
    IrSpectra* ir;
    int leader;
    int ncol;
    int irCh[16], outCh[16];
  };
  struct GroupInfo {   // a fused group (by leader), or a convolver on its own
    uint64_t sig = 1469598103934665603ull;
    int maxP = 0, nIn = 0, nOut = 0;
    const void* ir0 = nullptr;
    bool oneIr = true, tail = false, carried = false, fresh = true, noHist = false;
    // time-domain pre-mix (option "coarse_premix"): every member convolves with the same spectra and has the same channel
    // layout, so the group's inputs are added up in front of ONE set of transforms
    bool uniform = true, premix = false;
    int members = 0, nxr = 0, bInCh0 = 0, bSlots0 = 0;
    bool ts0 = false;
    int64_t hl0 = 0;
    struct Terms { std::vector<PremixTerm> in[32], hist[32]; };   // per input channel of the group
    std::unique_ptr<Terms> terms;                                 // (pre-mixed groups only)
  };
  std::vector<Views> chInOf;   // [position in dNodes]: chunk-long views of the node's input channels
  bool wideStrided = true;   // every 16-column term's spectra are h[0] + c x P x kCoarseBins
  std::vector<CoarseHandOver> fwdHandOver;   // a pending hand-over that rides in the first forward launch of this stage
  std::vector<PremixJob> pmJobs;
  std::vector<PremixTerm> pmTerms;
  size_t pmUsed = 0;       // bytes of the pre-mix arena handed out
  int64_t pmMaxN = 0;
  int pmHandOver = 0;   // hand-over jobs at the head of pmJobs
  double pmBytes = 0;
  std::vector<CoarseXRow> xrows;
  std::vector<CoarseHistJob> hjobs;
  std::vector<Piece> pieces;
  std::map<int, GroupInfo> groups;   // by leader
  const bool tails;
  int frameNext = 0;
  int64_t maxHist = 0;
  double histBytes = 0;
  std::map<int, double> carryBytes;   // row -> bytes of next-chunk history its forward transform also writes
  int nxAll = 0, G = 1;
  int gBegin[9] = {};
  std::vector<CoarseTerm> terms;
  // launches: by column count (1, 2, 4) x (terms with their own impulse responses | one impulse response for all terms), and
  // by the group whose transforms complete the job's inputs.  Class index = 2 * column class + shared.
  static constexpr int kCwOf[4] = {1, 2, 4, 16};   // column classes of the multiply-accumulate launches
  // Classes 8 .. 15: the same for jobs of more than kCoarseMaxP partitions (segmented sum: kernels of their own).
  std::vector<CoarseJob> jobs[16][8];
  int maxT[16] = {}, maxP[16] = {};
  int pbOf[16] = {4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4};   // largest of 4, 2, 1 dividing every job's partition count (the sweep's register block)
  double macBytes[16][8] = {}, macFlops[16][8] = {};
  double pmFlops = 0, invFlops = 0;
  std::map<std::pair<int, int>, std::vector<int>> outRows;   // (leader, channel) -> Y rows to sum
  int yNext = 0;
  std::vector<CoarseOut> outs;
  std::vector<int> ylist;
  double invBytes = 0;
  int yFrames = 0, invBlocks = 0;

  CoarseStage(Context& c_, Exec& ex_, const std::vector<int>& d, int64_t n_)
      : c(c_), ex(ex_), dNodes(d), n(n_), frames(n_ * kBlock), nT((int)((n_ * kBlock + kCoarseBlock - 1) / kCoarseBlock)), tails(c_.coarseTail) {}
  void resolveInputs();    // chunk-long input views of every node (materialised where the segments disagree)
  void classifyGroups();   // which groups are pre-mixed, carry a tail, can use the one the previous chunk left
  void buildRows();        // signals to transform (pre-mixed groups: one per channel), history hand-over, pieces (signal x columns)
  void addPieces(ConvolverS& nd, int leader, int nxr, const int* xFrame, const int* xIndex);
  void buildJobs();        // multiply-accumulate jobs and their terms
  void buildOutputs();     // inverse-transform outputs, tail buffers
  void enqueue();          // tables into the plan, launches
};

void CoarseStage::resolveInputs() {
  chInOf.resize(dNodes.size());
  for (size_t di = 0; di < dNodes.size(); di++) {
    const int id = dNodes[di];
    ConvolverS& nd = rec<ConvolverS>(*c.nodes[id]);
    const int64_t hl = nd.dHistLen;
    const Exec::ConvInRow ci = ex.convIn[id];
    Views& chIn = chInOf[di];
    chIn.assign(nd.bInCh, nullptr);
    auto viewOf = [&](size_t si, int ch) { return (ci[si].empty() || ch >= (int)ci[si].size()) ? (const float*)nullptr : ci[si][ch]; };
    for (int ch = 0; ch < nd.bInCh; ch++) {
      // a channel that shows the same view as an earlier one in every segment IS that channel (a mono signal copied to all
      // channels of an explicit input, AudioNodeInput.cs:201-213): one chunk-long view -- one materialised copy -- serves both
      int same = -1;
      for (int e = 0; e < ch && same < 0; e++) {
        bool eq = true;
        for (size_t si = 0; si < ex.segs.size() && eq; si++) eq = viewOf(si, e) == viewOf(si, ch);
        if (eq) same = e;
      }
      chIn[ch] = same >= 0 ? chIn[same] : convChunkInput(c, ex, ci, ch);
    }
    bool allSame = true;
    for (int ch = 1; ch < nd.bInCh; ch++) allSame = allSame && (chIn[ch] == chIn[0]);
    if (nd.bShared && !allSame) {   // the channels start to differ: every channel inherits the (so far common) history
      // (a plan entry like every other device action of the chunk: ordered with the chunk's launches, nothing is issued at plan time)
      if (const float* h0 = coarseHistory(nd, 0))
        for (int ch = 1; ch < nd.bInCh; ch++) {
          float* dst = nd.dHist[nd.dHistCur] + (size_t)ch * hl;
          hipStream_t st = c.stream;
          ex.plan.add(LK_OTHER, [=](uint8_t*) { GA_HIP(hipMemcpyAsync(dst, h0, (size_t)hl * sizeof(float), hipMemcpyDeviceToDevice, st)); });
          if (ch < (int)nd.dHistExt.size()) nd.dHistExt[ch] = {nullptr, -1};
        }
      if (nd.dHistZero && coarseHistory(nd, 0)) nd.dHistZero = false;   // (the copies above are the channels' histories now)
      nd.bShared = false;
    }
  }
}

void CoarseStage::classifyGroups() {
  // ---- carried tails (option "coarse_tail"): every output of the stage keeps, from chunk to chunk, what the input so far adds to
  // the samples behind the chunk's end.  While a group of fused convolvers is the same as in the previous chunk its members need
  // no input history in front of the chunk: their windows start at the chunk (u = 0) and the previous chunk's tail is added to
  // the output instead -- P' - 1 fewer transforms per signal and chunk.  Any change (member set, impulse responses, channel
  // modes, a chunk in between that did not run this stage) falls back to the input histories, which are kept up to date either way.
  {
    auto mix = [](uint64_t& h, uint64_t v) { h = (h ^ v) * 1099511628211ull; };
    for (int id : dNodes) {
      ConvolverS& nd = rec<ConvolverS>(*c.nodes[id]);
      GroupInfo& g = groups[nd.dLeader >= 0 ? nd.dLeader : id];
      mix(g.sig, (uint64_t)id);
      mix(g.sig, (uint64_t)(uintptr_t)nd.ir.get());
      mix(g.sig, (uint64_t)nd.bInCh | ((uint64_t)nd.bSlots << 8) | ((uint64_t)nd.isTrueStereo << 16) | ((uint64_t)nd.bShared << 17) |
                     ((uint64_t)nd.ir->coarseP << 24));
      g.maxP = std::max(g.maxP, nd.ir->coarseP);
      g.fresh = g.fresh && nd.dHistZero;   // no member has seen input yet: nothing in front of the chunk either
      g.nIn += nd.bShared ? 1 : nd.bInCh;
      if (!g.ir0) g.ir0 = nd.ir.get();
      g.oneIr = g.oneIr && g.ir0 == nd.ir.get();
      g.nOut = std::max(g.nOut, nd.isTrueStereo ? 2 : nd.bSlots);
      const int nxr = nd.bShared ? 1 : nd.bInCh;
      if (g.members++ == 0) {
        g.nxr = nxr;
        g.bInCh0 = nd.bInCh;
        g.bSlots0 = nd.bSlots;
        g.ts0 = nd.isTrueStereo;
        g.hl0 = nd.dHistLen;
      } else {
        g.uniform = g.uniform && g.nxr == nxr && g.bInCh0 == nd.bInCh && g.bSlots0 == nd.bSlots && g.ts0 == nd.isTrueStereo && g.hl0 == nd.dHistLen;
      }
    }
    for (auto& kv : groups) {
      ConvolverS& ld = rec<ConvolverS>(*c.nodes[kv.first]);
      // a tail costs P' more inverse transforms per output channel and chunk and saves P' - 2 forward transforms per input row:
      // worth it for sums of many signals, not for a convolver on its own.  The P' more output blocks are nearly free in the
      // reduction kernel (one impulse response for the whole group); the general kernel skips the partition blocks whose windows
      // lie behind the chunk (all zero), so a group of private impulse responses multiplies exactly the products it would have
      // multiplied with the histories in front -- but measured it does not pay (ga_engine.hpp): option "coarse_tail_private", off
      kv.second.premix = c.coarsePremix && kv.second.members >= 2 && kv.second.oneIr && kv.second.uniform && kv.second.nxr <= 32;
      // (a pre-mixed group always keeps its tail: reading every member's history again would cost members x (P' - 1) blocks)
      kv.second.tail = tails && (kv.second.oneIr || c.coarseTailPrivate) &&
                       (kv.second.premix || (int64_t)kv.second.nIn * (kv.second.maxP - 2) >= (int64_t)kv.second.nOut * kv.second.maxP);
      kv.second.carried = kv.second.tail && ld.dTail[0] && ld.dTailSeq + 1 == c.chunkSeq && ld.dTailSig == kv.second.sig &&
                          ld.dTailLen == (int64_t)(kv.second.maxP + 1) * kCoarseBlock;
      kv.second.noHist = kv.second.carried || (kv.second.tail && kv.second.fresh);
    }
  }
}

// columns of a node's input rows: discrete -> slot c reads input c, IR channel c, output c ; true stereo -> (L,h0,outL) (L,h1,outR)
// (R,h2,outL) (R,h3,outR)  (ConvolverNode.cs:127-151).  Pieces of 4, 2, 1 columns per row.
void CoarseStage::addPieces(ConvolverS& nd, int leader, int nxr, const int* xFrame, const int* xIndex) {
  IrSpectra& ir = *nd.ir;
  for (int xc = 0; xc < nxr; xc++) {
    int cols[32][2], ncols = 0;
    for (int slot = 0; slot < nd.bSlots; slot++) {
      const int inc = nd.isTrueStereo ? (slot >> 1) : slot;
      if (!(nd.bShared || inc == xc)) continue;
      cols[ncols][0] = slot;                               // slot index == IR channel index in both modes
      cols[ncols][1] = nd.isTrueStereo ? (slot & 1) : slot;
      ncols++;
    }
    // 16 columns of one signal at once where the group's terms have impulse responses of their own (the general kernel's 16-column
    // instance: the signal's frames are staged once for all of them) and its double-buffered spectra fit the LDS (P' <= 4)
    const GroupInfo& gi = groups[leader];
    const bool wide = !gi.oneIr && ir.coarseP <= 4 && c.coarseWide;
    for (int c0 = 0; c0 < ncols;) {
      const int left = ncols - c0;
      const int w = (wide && left >= 16) ? 16 : (left >= 4 ? 4 : (left >= 2 ? 2 : 1));
      Piece pc{};
      pc.frame0 = xFrame[xc];
      pc.xrow = xIndex[xc];
      pc.u0 = xrows[xIndex[xc]].u0;
      pc.P = ir.coarseP;
      pc.ir = &ir;
      pc.leader = leader;
      pc.ncol = w;
      for (int j = 0; j < w; j++) {
        pc.irCh[j] = cols[c0 + j][0];
        pc.outCh[j] = cols[c0 + j][1];
      }
      pieces.push_back(pc);
      c0 += w;
    }
  }
}

void CoarseStage::buildRows() {
  for (size_t di = 0; di < dNodes.size(); di++) {
    const int id = dNodes[di];
    ConvolverS& nd = rec<ConvolverS>(*c.nodes[id]);
    IrSpectra& ir = *nd.ir;
    const int P = ir.coarseP;
    if (P < 1 || P > kCoarseMaxParts) fail(GA_ERR_INVALID_OPERATION, "internal: coarse partition count out of range");
    const int64_t hl = nd.dHistLen;
    GroupInfo& gi0 = groups[nd.dLeader >= 0 ? nd.dLeader : id];
    const bool carried = gi0.noHist;   // no windows in front of the chunk
    const Views& chIn = chInOf[di];
    const int nxr = nd.bShared ? 1 : nd.bInCh;
    c.stats.mac_flops_total += 8.0 * ir.P * kBins * (double)nd.bSlots * (double)n;
    c.stats.mac_bytes_total += ((double)ir.P * kBins * 8.0 + kBins * 8.0 + 512.0) * nd.bSlots * (double)n;
    if (gi0.premix) {
      // a member of a pre-mixed group: nothing to transform for it; its samples join the group's sum and its own history of the
      // next chunk is written on the way (or by a copy job where that is not possible)
      for (int ch = 0; ch < nxr; ch++) {
        const float* oldHist = coarseHistory(nd, ch);
        float* nextHist = nd.dHist[nd.dHistCur ^ 1] + (size_t)ch * hl;
        PremixTerm t{chIn[ch], nullptr};
        if (coarseHistoryStays(c, nd, ch, chIn[ch], frames)) {
          // (the next chunk's history is a span of the member's sample buffer)
        } else if (c.coarseCarry && chIn[ch] && frames >= hl && ((uintptr_t)nextHist & 15) == 0) {
          t.carry = nextHist;
          pmBytes += (double)hl * 4.0;
        } else {
          hjobs.push_back(CoarseHistJob{oldHist, chIn[ch], nextHist, hl, frames});
          maxHist = std::max(maxHist, hl);
          histBytes += 2.0 * (double)hl * 4.0;
        }
        if (!gi0.terms) gi0.terms = std::make_unique<GroupInfo::Terms>();
        gi0.terms->in[ch].push_back(t);
        if (!carried) gi0.terms->hist[ch].push_back(PremixTerm{oldHist, nullptr});
      }
      nd.dHistCur ^= 1;
      nd.dHistZero = false;
      continue;
    }
    int xFrame[32], xIndex[32];
    for (int ch = 0; ch < nxr; ch++) {
      CoarseXRow r;
      const float* oldHist = coarseHistory(nd, ch);   // (kept up to date in every mode)
      r.hist = carried ? nullptr : oldHist;
      r.in = chIn[ch];
      r.nvalid = frames;
      r.frame0 = frameNext;
      // windows u0 .. u_last: with carried tails the last one is u = nT ([last block | nothing yet]: it feeds the outputs behind
      // the chunk's end), and a group that continues needs none in front of the chunk
      r.u0 = carried ? 0 : -(P - 1);
      r.n_frames = (gi0.tail ? nT + 1 : nT) - r.u0;
      r.hist_len = (int)hl;
      r.flags = 0;
      r.scale = 1.0f;
      xFrame[ch] = frameNext;
      xIndex[ch] = (int)xrows.size();
      frameNext += r.n_frames;
      // the next chunk's history: the last hl samples of [history | input].  When they all come from this chunk's input the
      // forward kernel writes them while it holds the samples (ga_kernels.hpp, CoarseXRow::carry); otherwise a copy job.
      float* nextHist = nd.dHist[nd.dHistCur ^ 1] + (size_t)ch * hl;
      r.carry = nullptr;
      r.carry_from = 0;
      if (coarseHistoryStays(c, nd, ch, r.in, frames)) {
        // (the next chunk's history is a span of the sample buffer the input aliases)
      } else if (c.coarseCarry && r.in && frames >= hl && (((uintptr_t)r.in | (uintptr_t)nextHist) & 15) == 0) {
        r.carry = nextHist;
        r.carry_from = frames - hl;
        carryBytes[(int)xrows.size()] = (double)hl * 4.0;
      } else {
        hjobs.push_back(CoarseHistJob{oldHist, r.in, nextHist, hl, frames});
        maxHist = std::max(maxHist, hl);
        histBytes += 2.0 * (double)hl * 4.0;
      }
      xrows.push_back(r);
    }
    nd.dHistCur ^= 1;
    nd.dHistZero = false;
    addPieces(nd, nd.dLeader >= 0 ? nd.dLeader : id, nxr, xFrame, xIndex);
  }
  // ---- pre-mixed groups: one mixed signal [history | chunk] per input channel, transformed like a single convolver's input ----
  for (auto& kv : groups) {
    GroupInfo& g = kv.second;
    if (!g.premix) continue;
    ConvolverS& ld = rec<ConvolverS>(*c.nodes[kv.first]);
    const int64_t hl = g.hl0;
    int xFrame[32], xIndex[32];
    for (int ch = 0; ch < g.nxr; ch++) {
      const size_t bytes = (size_t)(hl + frames) * sizeof(float);
      // (two halves: the forward transforms of the previous chunk may still read the other one, option "coarse_tail_stream")
      const size_t half = (c.coarseM.bytes / 2) & ~(size_t)255;
      if (pmUsed + bytes > half) fail(GA_ERR_INVALID_OPERATION, "internal: the pre-mix arena is too small for the plan");
      float* mixed = (float*)((char*)c.coarseM.p + ((c.chunkSeq & 1) ? half : 0) + pmUsed);
      pmUsed += (bytes + 255) & ~(size_t)255;
      auto job = [&](float* out, const std::vector<PremixTerm>& tv, int64_t len, int64_t carryFrom) {
        PremixJob j{out, (int)pmTerms.size(), 0, len, carryFrom, 1, 0};
        for (const PremixTerm& t : tv) {
          if (!t.in) continue;   // (silent: adds nothing, and has no carry)
          pmTerms.push_back(t);
          j.nterms++;
          if ((uintptr_t)t.in & 15) j.flags &= ~1;
          if (t.carry) j.flags |= 2;
          pmBytes += (double)len * 4.0;
          pmFlops += (double)len * 4.0;   // (compensated summation: four operations per sample)
        }
        pmJobs.push_back(j);
        pmMaxN = std::max(pmMaxN, len);
        pmBytes += (double)len * 4.0;
      };
      if (!g.terms) g.terms = std::make_unique<GroupInfo::Terms>();
      if (!g.noHist) job(mixed, g.terms->hist[ch], hl, hl);
      job(mixed + hl, g.terms->in[ch], frames, std::max<int64_t>(0, frames - hl));
      CoarseXRow r{};
      r.hist = g.noHist ? nullptr : mixed;
      r.in = mixed + hl;
      r.nvalid = frames;
      r.frame0 = frameNext;
      r.u0 = g.noHist ? 0 : -(g.maxP - 1);
      r.n_frames = (g.tail ? nT + 1 : nT) - r.u0;
      r.hist_len = (int)hl;
      r.flags = 0;
      r.scale = 1.0f;
      r.carry = nullptr;
      r.carry_from = 0;
      xFrame[ch] = frameNext;
      xIndex[ch] = (int)xrows.size();
      frameNext += r.n_frames;
      xrows.push_back(r);
    }
    addPieces(ld, kv.first, g.nxr, xFrame, xIndex);
    c.stats.coarse_premixed_signals += (int64_t)g.members * g.nxr;
  }
  // the previous chunk's bus on its way to the caller's page-locked rows (Context::pendingHandOver): one-term jobs at the head of
  // this launch -- their workgroups write over PCIe while the others stream the members' samples from HBM
  // option "coarse_tail_stream": this stage may run behind its pre-mix on stream2 (Context::chunkExecute decides), where the
  // previous chunk's inverse transforms wrote that bus -- then the hand-over rides in the forward launch, on the same stream
  c.tailCandidate = c.tailWanted && !pmJobs.empty() && hjobs.empty() && !c.coarseOverlap && ex.plan.launches.empty();
  if (c.tailCandidate && !c.pendingHandOver.empty() && !xrows.empty()) {
    for (const Context::HandOver& h : c.pendingHandOver) fwdHandOver.push_back(CoarseHandOver{h.src, h.dst_dev, h.n});
    c.pendingHandOver.clear();
    c.stats.deferred_handovers++;
  } else if (!pmJobs.empty() && !c.pendingHandOver.empty()) {
    std::vector<PremixJob> head;
    for (const Context::HandOver& h : c.pendingHandOver) {
      head.push_back(PremixJob{h.dst_dev, (int)pmTerms.size(), 1, h.n, h.n, 1 | 4, 0});
      pmTerms.push_back(PremixTerm{h.src, nullptr});
      pmMaxN = std::max(pmMaxN, h.n);
      pmBytes += 2.0 * (double)h.n * 4.0;
    }
    pmJobs.insert(pmJobs.begin(), head.begin(), head.end());
    pmHandOver = (int)head.size();
    c.pendingHandOver.clear();
    c.stats.deferred_handovers++;
  } else if (!c.pendingHandOver.empty() && !xrows.empty()) {   // no pre-mix launch: they ride in the stage's first forward launch
    for (const Context::HandOver& h : c.pendingHandOver) fwdHandOver.push_back(CoarseHandOver{h.src, h.dst_dev, h.n});
    c.pendingHandOver.clear();
    c.stats.deferred_handovers++;
  }
  ex.flushLevel();   // (materialised inputs)
}

void CoarseStage::buildJobs() {
  // ---- jobs: pieces with the same (leader, output channels, partitions) accumulate into the same Y rows ----
  struct Key {
    int leader, P, ncol;
    std::array<int, 16> out;
    bool operator<(const Key& o) const { return std::tie(leader, P, ncol, out) < std::tie(o.leader, o.P, o.ncol, o.out); }
  };
  std::map<Key, std::vector<const Piece*>> byKey;
  for (const Piece& pc : pieces) {
    Key k{pc.leader, pc.P, pc.ncol, {}};
    k.out.fill(-1);
    for (int j = 0; j < pc.ncol; j++) k.out[j] = pc.outCh[j];
    byKey[k].push_back(&pc);
  }
  // groups of signals: the multiply-accumulate jobs of group g run (second stream) while group g + 1 is transformed
  nxAll = (int)xrows.size();
  G = !c.coarseOverlap ? 1 : (nxAll >= 256 ? 4 : (nxAll >= 64 ? 2 : 1));
  auto groupOf = [&](int xrow) { return std::min(G - 1, (int)((int64_t)xrow * G / std::max(nxAll, 1))); };
  for (int g = 0; g <= G; g++) gBegin[g] = 0;
  for (int x = 0; x < nxAll; x++) gBegin[groupOf(x) + 1] = x + 1;
  for (int g = 1; g <= G; g++) gBegin[g] = std::max(gBegin[g], gBegin[g - 1]);
  for (auto& kv : byKey) {
    const Key& k = kv.first;
    const int cw = k.ncol, ci = cw == 1 ? 0 : (cw == 2 ? 1 : (cw == 4 ? 2 : 3));
    const auto& pv = kv.second;
    for (size_t p0 = 0; p0 < pv.size(); p0 += kVoicesPerJob) {
      const size_t p1 = std::min(pv.size(), p0 + kVoicesPerJob);
      const int term0 = (int)terms.size();
      bool shared = true;
      int lastX = 0;
      // more than kCoarseMaxP partitions: the sum runs in segments of kCoarseMaxP partitions inside the job (ga_coarse.hip,
      // coarse_sum_seg_kernel / coarse_mac_seg_kernel); the accumulators stay in registers over all of them
      const bool seg = k.P > kCoarseMaxP;
      for (size_t i = p0; i < p1; i++) {
        const Piece& pc = *pv[i];
        CoarseTerm t{};
        t.frame0 = pc.frame0 - (pc.u0 + (pc.P - 1));   // frame the window u = -(P - 1) would have (the kernels index from there)
        if (seg) t.frame0 = pc.frame0 - pc.u0;         // segmented sum: the frame the window u = 0 would have
        for (int j = 0; j < 16; j++) t.h[j] = nullptr;
        for (int j = 0; j < cw; j++) t.h[j] = pc.ir->coarse + (size_t)pc.irCh[j] * pc.ir->coarseStride * kCoarseBins;
        if (i > p0)
          for (int j = 0; j < cw; j++) shared = shared && (t.h[j] == terms[term0].h[j]);
        terms.push_back(t);
        lastX = std::max(lastX, pc.xrow);
      }
      if (cw == 16) {
        shared = false;   // (the reduction kernel has no 16-column instance)
        for (size_t i = term0; i < terms.size(); i++)   // the matrix-core kernel addresses the columns' spectra from h[0]
          for (int j = 1; j < 16; j++) wideStrided = wideStrided && terms[i].h[j] == terms[i].h[0] + (size_t)j * k.P * kCoarseBins;
      }
      if (seg && cw == 16) fail(GA_ERR_INVALID_OPERATION, "internal: 16-column piece with a segmented partition sum");
      if (seg && !shared) terms.resize(term0);   // (the general kernel's terms are (signal, segment) pairs, listed per job below)
      const int grp = groupOf(lastX);
      const int yrow0 = yNext;
      yNext += cw;
      for (int j = 0; j < cw; j++) outRows[{k.leader, k.out[j]}].push_back(yrow0 + j);
      const int jb = shared ? kCoarseSumJobBlocks(cw) : kCoarseJobBlocks(cw);   // (the two kernels' job sizes)
      const GroupInfo& gi = groups[k.leader];
      const int nTo = gi.tail ? nT + gi.maxP : nT;   // output blocks: the chunk's, and with a tail those the chunk's input still reaches
      for (int t0 = 0; t0 < nTo; t0 += jb) {
        CoarseJob jb_{};
        jb_.term0 = term0;
        jb_.n_terms = (int)(p1 - p0);
        jb_.P = k.P;
        jb_.t0 = t0;
        jb_.n_t = std::min(jb, nTo - t0);
        jb_.yrow0 = yrow0;
        jb_.shared_h = shared ? 1 : 0;
        jb_.u_lo = gi.noHist ? 0 : -(k.P - 1);
        jb_.u_hi = gi.tail ? nT : nT - 1;
        const int cj = 2 * ci + (shared ? 1 : 0) + (seg ? 8 : 0);
        if (seg) {
          // per segment: the windows t - off - p the job's blocks reach, those of them that exist, the partitions multiplied
          // (stage_bytes / stage_flops count what is executed: a segment's frames are fetched once per segment)
          double xFrames = 0, parts = 0;
          if (!shared) jb_.term0 = (int)terms.size();
          int npairs = 0;
          auto addSegment = [&](const Piece* pc, int off, bool force) {   // pc: the general kernel's (signal, segment) pair
            const int np = pc ? std::min(kCoarseMaxP, (k.P - off + 3) / 4 * 4) : std::min(kCoarseMaxP, k.P - off);
            const int wLo = std::max(jb_.u_lo, t0 - off - (kCoarseMaxP - 1)), wHi = std::min(jb_.u_hi, t0 + jb_.n_t - 1 - off);
            if (!force && (wLo > wHi || t0 - off - (np - 1) > jb_.u_hi)) return;   // none of the segment's windows exists
            xFrames += (double)std::max(0, wHi - wLo + 1) * (pc ? 1 : jb_.n_terms);
            parts += np;
            npairs++;
            if (!pc) return;
            CoarseTerm t{};
            t.frame0 = pc->frame0 - pc->u0 - off - (kCoarseMaxP - 1);
            t.pad_ = off + 256 * np;
            for (int j = 0; j < 16; j++) t.h[j] = nullptr;
            for (int j = 0; j < cw; j++) t.h[j] = pc->ir->coarse + ((size_t)pc->irCh[j] * pc->ir->coarseStride + off) * kCoarseBins;
            terms.push_back(t);
          };
          for (size_t i = shared ? p1 - 1 : p0; i < p1; i++)
            for (int off = 0; off < k.P; off += kCoarseMaxP) addSegment(shared ? nullptr : pv[i], off, false);
          if (npairs == 0) addSegment(shared ? nullptr : pv[p0], 0, true);   // (a job of zero rows still writes its Y blocks)
          if (!shared) jb_.n_terms = (int)terms.size() - jb_.term0;
          jobs[cj][grp].push_back(jb_);
          maxT[cj] = std::max(maxT[cj], jb_.n_t);
          maxP[cj] = std::max(maxP[cj], k.P);
          macBytes[cj][grp] += xFrames * kCoarseBins * 8.0 + (t0 == 0 ? (double)(shared ? 1 : (p1 - p0)) * k.P * cw * kCoarseBins * 8.0 : 0.0) +
                               (double)cw * jb_.n_t * kCoarseBins * 8.0;
          macFlops[cj][grp] += shared ? (xFrames * 2.0 + parts * jb_.n_t * cw * 8.0) * kCoarseBins : parts * jb_.n_t * cw * 8.0 * kCoarseBins;
          continue;
        }
        jobs[cj][grp].push_back(jb_);
        maxT[cj] = std::max(maxT[cj], jb_.n_t);
        maxP[cj] = std::max(maxP[cj], k.P);
        while (k.P % pbOf[cj]) pbOf[cj] >>= 1;
        const int fread = std::max(0, std::min(jb_.u_hi, t0 + jb_.n_t - 1) - std::max(jb_.u_lo, t0 - (k.P - 1)) + 1);   // frames that exist
        // (the spectra of the terms are necessary bytes ONCE: the block ranges of one group of terms are neighbours in the grid and
        // the second range finds them in the L2 -- PMC: profiles/r03_config5_pmc_hbm_traffic.json)
        macBytes[cj][grp] += (double)jb_.n_terms * fread * kCoarseBins * 8.0 +
                             (t0 == 0 ? (double)(shared ? 1 : jb_.n_terms) * k.P * cw * kCoarseBins * 8.0 : 0.0) + (double)cw * jb_.n_t * kCoarseBins * 8.0;
        // complex multiply-adds (8 flops): every term's products in the general kernel; in the reduction the terms' frames are
        // added up first (2 flops per complex value) and the sum is multiplied once
        macFlops[cj][grp] += shared ? ((double)jb_.n_terms * fread * 2.0 + (double)k.P * jb_.n_t * cw * 8.0) * kCoarseBins
                                    : (double)jb_.n_terms * k.P * jb_.n_t * cw * 8.0 * kCoarseBins;
      }
    }
  }
}

void CoarseStage::buildOutputs() {
  int maxPAll = 0;
  for (auto& kv : groups)
    if (kv.second.tail) maxPAll = std::max(maxPAll, kv.second.maxP);
  yFrames = nT + maxPAll;   // coarse blocks per Y row (rows of groups with a shorter or no tail leave their end unused)
  invBlocks = nT;
  if (tails) {   // tail buffers live with the group's leader: [2][channels][tail_len], read one, write the other
    std::map<int, int> chOf;
    for (auto& kv : outRows) chOf[kv.first.first] = std::max(chOf[kv.first.first], kv.first.second + 1);
    for (auto& kv : groups) {
      if (!kv.second.tail) continue;
      ConvolverS& ld = rec<ConvolverS>(*c.nodes[kv.first]);
      const int64_t len = (int64_t)(kv.second.maxP + 1) * kCoarseBlock;
      const int nch = chOf.count(kv.first) ? chOf[kv.first] : 0;
      if (nch == 0) continue;
      if (!ld.dTail[0] || ld.dTailLen != len || ld.dTailCh != nch) {
        if (kv.second.carried) fail(GA_ERR_INVALID_OPERATION, "internal: a carried tail changed its shape");
        c.syncStream();
        for (int b = 0; b < 2; b++) {
          if (ld.dTail[b]) c.dfree(ld.dTail[b], (size_t)ld.dTailLen * ld.dTailCh * sizeof(float));
          ld.dTail[b] = (float*)c.dalloc((size_t)len * nch * sizeof(float));
        }
        ld.dTailLen = len;
        ld.dTailCh = nch;
        ld.dTailCur = 0;
      }
    }
  }
  for (auto& kv : outRows) {
    CoarseOut o{};
    o.out = ex.nodeOut(kv.first.first, kv.first.second);
    o.nvalid = frames;
    o.y0 = (int)ylist.size();
    o.ny = (int)kv.second.size();
    o.n_y = nT;
    if (groups[kv.first.first].tail) {
      ConvolverS& ld = rec<ConvolverS>(*c.nodes[kv.first.first]);
      const GroupInfo& gi = groups[kv.first.first];
      o.n_y = nT + gi.maxP;
      o.tail_len = ld.dTailLen;
      o.tail_in = gi.carried ? ld.dTail[ld.dTailCur] + (size_t)kv.first.second * ld.dTailLen : nullptr;
      o.tail_out = ld.dTail[ld.dTailCur ^ 1] + (size_t)kv.first.second * ld.dTailLen;
      invBlocks = std::max(invBlocks, (int)((frames + o.tail_len + kCoarseBlock - 1) / kCoarseBlock));
      invBytes += (double)o.tail_len * 4.0 * (gi.carried ? 2.0 : 1.0);
      if (gi.carried) c.stats.coarse_carried_outputs++;
    }
    ylist.insert(ylist.end(), kv.second.begin(), kv.second.end());
    outs.push_back(o);
    invBytes += (double)o.ny * o.n_y * kCoarseBins * 8.0 + (double)frames * 4.0;
    invFlops += (double)o.n_y * (kCoarseTransformFlops + (double)o.ny * 2.0 * kCoarseBins);
  }
  if (tails)
    for (auto& kv : groups) {   // this chunk's tails are the next chunk's, if the group is still the same then
      ConvolverS& ld = rec<ConvolverS>(*c.nodes[kv.first]);
      if (!kv.second.tail || !ld.dTail[0]) continue;
      ld.dTailCur ^= 1;
      ld.dTailSig = kv.second.sig;
      ld.dTailSeq = c.chunkSeq;
    }
  if ((size_t)frameNext * kCoarseBins * sizeof(float2) > c.coarseX.bytes || (size_t)yNext * yFrames * kCoarseBins * sizeof(float2) > c.coarseY.bytes)
    fail(GA_ERR_INVALID_OPERATION, "internal: coarse spectra arenas are too small for the plan");

}

void CoarseStage::enqueue() {
  // (the launches below run after this object is gone: they capture locals, never members)
  const int G = this->G, yFrames = this->yFrames, invBlocks = this->invBlocks, nxAll = this->nxAll;
  const double invBytes = this->invBytes, histBytes = this->histBytes;
  const size_t xo = ex.plan.putv(xrows), ho = ex.plan.putv(hjobs), to = ex.plan.putv(terms), oo = ex.plan.putv(outs), yo = ex.plan.putv(ylist);
  const size_t pjo = ex.plan.putv(pmJobs), pto = ex.plan.putv(pmTerms), fho = ex.plan.putv(fwdHandOver);
  const int nfh = (int)fwdHandOver.size();
  const int npm = (int)pmJobs.size(), npmHandOver = this->pmHandOver, pmWgsPerCu = c.coarsePremixWgsPerCu;
  const int64_t pmMaxN = this->pmMaxN;
  const double pmBytes = this->pmBytes, pmFlops = this->pmFlops, invFlops = this->invFlops;
  struct MacLaunch { size_t off; int nj, cw, mt, mp, pb, grp; bool ap; double bytes, flops; };
  const bool matrixCores = c.coarseMfma && wideStrided;
  std::vector<MacLaunch> macs;
  for (int g = 0; g < G; g++)
    for (int i = 0; i < 16; i++) {
      if (jobs[i][g].empty()) continue;
      macs.push_back(MacLaunch{ex.plan.putv(jobs[i][g]), (int)jobs[i][g].size(), kCwOf[(i & 7) >> 1], maxT[i], maxP[i], pbOf[i], g, (i & 1) == 0,
                               macBytes[i][g], macFlops[i][g]});
      c.stats.mac_launches += 1;
    }
  hipStream_t st = c.stream;
  float2* X = (float2*)c.coarseX.p;
  float2* Y = (float2*)c.coarseY.p;
  const float2* tw16 = c.twiddles16(4096);
  const float2* twFwd = c.twiddles16pw();
  const float2* twab = c.coarseTwab();
  const int nh = (int)hjobs.size(), no = (int)outs.size();
  // per group: rows, longest row, bytes, windows per workgroup (long runs fetch every input sample once; keep >= ~4
  // workgroups per CU's worth of parallelism)
  struct FwdLaunch { int x0, nx, maxFrames, run; double bytes, flops; };
  std::vector<FwdLaunch> fwds;
  for (int g = 0; g < G; g++) {
    FwdLaunch f{this->gBegin[g], this->gBegin[g + 1] - this->gBegin[g], 0, 1, 0.0, 0.0};
    for (int x = f.x0; x < f.x0 + f.nx; x++) {
      f.maxFrames = std::max(f.maxFrames, xrows[x].n_frames);
      f.bytes += (double)(xrows[x].n_frames + 1) * kCoarseBlock * 4.0 + (double)xrows[x].n_frames * kCoarseBins * 8.0;
      f.flops += (double)xrows[x].n_frames * kCoarseTransformFlops;
      if (auto it = carryBytes.find(x); it != carryBytes.end()) f.bytes += it->second;
    }
    while (f.run < 16 && (int64_t)nxAll * ((f.maxFrames + 2 * f.run - 1) / (2 * f.run)) >= 1024) f.run *= 2;
    if (f.run >= 8) {   // equal runs of about 12 windows (measured on config 3: 10, 12 and 20 per run beat 16 + a short last run by 2.5 %)
      const int k = (f.maxFrames + 11) / 12;
      f.run = (f.maxFrames + k - 1) / k;
    }
    if (const char* e = expenv("GA_COARSE_RUN")) f.run = std::max(1, atoi(e));   // measurements only
    fwds.push_back(f);
  }
  if (G > 1) c.ensureOverlapStream();
  Context* cp = &c;
  ex.plan.add(GA_STAGE_COARSE_SECTION, [=](uint8_t* base) {
    // one piece of the section: a launch with its own profile events (the two stages overlap on two streams)
    auto timed = [&](hipStream_t sx, int kind, double bytes, double flops, const std::function<const char*()>& launch) {
      hipEvent_t e0 = nullptr, e1 = nullptr;
      if (cp->profileNow) {
        GA_HIP(hipEventCreate(&e0));
        GA_HIP(hipEventCreate(&e1));
        GA_HIP(hipEventRecord(e0, sx));
      }
      cp->noteKernel(kind, launch());
      if (cp->profileNow) {
        GA_HIP(hipEventRecord(e1, sx));
        cp->extraProf.push_back(Context::ExtraProf{e0, e1, kind, bytes});
      }
      cp->stats.kernel_launches++;
      cp->stats.stage_launches[kind]++;
      cp->stats.stage_bytes[kind] += bytes;
      cp->stats.stage_flops[kind] += flops;
    };
    if (npm > 0)
      timed(cp->stream, LK_CPREMIX, pmBytes, pmFlops, [&] { return launch_coarse_premix(st, (const PremixJob*)(base + pjo), npm, npmHandOver, (const PremixTerm*)(base + pto), pmMaxN, pmWgsPerCu); });
    // (option "coarse_tail_stream": everything behind the pre-mix goes to stream2, G == 1)
    hipStream_t ts = cp->tailStreamNow();
    if (cp->tailActive) {
      GA_HIP(hipEventRecord(cp->premixEv, cp->stream));
      GA_HIP(hipStreamWaitEvent(ts, cp->premixEv, 0));
    }
    hipStream_t s2 = G > 1 ? cp->stream2 : ts;
    for (int g = 0; g < G; g++) {
      const FwdLaunch& f = fwds[g];
      if (f.nx > 0)
        timed(ts, LK_CFWD, f.bytes, f.flops, [&] {
          return launch_coarse_fwd(ts, (const CoarseXRow*)(base + xo) + f.x0, f.nx, f.maxFrames, f.run, X, twFwd, twab,
                                   (const CoarseHandOver*)(base + fho), g == 0 ? nfh : 0);
        });
      if (G > 1) {
        GA_HIP(hipEventRecord(cp->dGroupEv[g], ts));
        GA_HIP(hipStreamWaitEvent(s2, cp->dGroupEv[g], 0));
      }
      for (const MacLaunch& m : macs)
        if (m.grp == g)
          timed(s2, LK_CMAC, m.bytes, m.flops, [&] {
            return launch_coarse_mac(s2, (const CoarseJob*)(base + m.off), m.nj, (const CoarseTerm*)(base + to), X, Y, yFrames, m.cw, m.mt, m.mp, m.ap, m.pb,
                                     matrixCores);
          });
    }
    if (G > 1) {   // join: the inverse transforms (and the next chunk's forward transforms, which reuse X) wait for every job
      GA_HIP(hipEventRecord(cp->dJoinEv, s2));
      GA_HIP(hipStreamWaitEvent(ts, cp->dJoinEv, 0));
    }
  });
  ex.plan.add(LK_CINV, [=](uint8_t* base) {
    cp->noteKernel(LK_CINV, launch_coarse_inv(cp->tailStreamNow(), (const CoarseOut*)(base + oo), no, invBlocks, (const int*)(base + yo), Y, yFrames, tw16, twab));
  }, invBytes, invFlops);
  const int64_t mh = maxHist;
  if (nh > 0) ex.plan.add(LK_CHIST, [=](uint8_t* base) { launch_coarse_hist(st, (const CoarseHistJob*)(base + ho), nh, mh); }, histBytes);
}
}  // namespace

static void planCoarseStage(Context& c, Exec& ex, const std::vector<int>& dNodes, int64_t n) {
  CoarseStage s(c, ex, dNodes, n);
  s.resolveInputs();
  s.classifyGroups();
  s.buildRows();
  s.buildJobs();
  s.buildOutputs();
  s.enqueue();
}

// When everything the destination receives in this chunk is ONE fused group of formulation D convolvers (or a single one) with
// the bus's channel count, the group's inverse transforms write the bus themselves: the leader's output slabs ARE the bus
// rows (the caller's device rows or page-locked host rows when Context::render set busTarget), and the destination's mix -- a
// copy of one term -- disappears (Exec::resolveInSeg skips a forced target that already holds its only term).
void Context::aliasBusToLeader(ChunkRun& r) {
  Exec& ex = *r.ex;
  int leader = -1, nch = 0;
  for (const Segment& sg : r.segs) {
    if (sg.nodes.empty() || sg.nodes.back().id != 0 || sg.nodes.back().ins.empty()) return;   // (node 0 is the destination)
    const InSeg& is = sg.nodes.back().ins[0];
    for (const TermS& t : is.terms) {
      if (nodes[t.node]->type != GA_NODE_CONVOLVER) return;
      const ConvolverS& nd = rec<ConvolverS>(*nodes[t.node]);
      if (!nd.ir || nd.convPath != 4 || nd.dLeader < 0 || t.out != 0 || t.ch != is.bufCh) return;
      if (leader < 0) {
        leader = nd.dLeader;
        nch = is.bufCh;
      } else if (leader != nd.dLeader || nch != is.bufCh) {
        return;
      }
    }
  }
  if (leader < 0 || nch < 1 || nch > (int)busSlabs.size()) return;
  const ConvolverS& ld = rec<ConvolverS>(*nodes[leader]);
  if (ld.outputs.empty() || ld.outputs[0].connectedInputs.size() != 1) return;
  const InRef& to = ld.outputs[0].connectedInputs[0];
  if (to.node != 0 || to.input != 0) return;
  for (int ch = 0; ch < nch; ch++) ex.setNodeOut(leader, ch, busTarget[ch] ? busTarget[ch] : busSlabs[ch]);
}

// ======================================================================================================
// option "conv_migrate": a convolver on formulation D becomes sensitive -> the B / C state layout, evaluated on R
// ======================================================================================================
// Formulation D's state is the node's last coarseP x 8192 input samples, and that is everything R's state is a function of: the
// spectra history is the forward transform of the last P - 1 blocks, the overlap is the second half of block T-1's inverse
// transform (T = first block of this chunk), whose partition sum reads blocks T-P .. T-1.  This pass only moves the node: it
// gets the private stores, notes where block T-P of every input channel lies and hands D's stores to the retire list (freed after
// the stream has run the rebuild, Context::freeRetired); planConvMigration enqueues the rebuild in front of the first convolver stage.
void Context::migrateConvolvers(const std::vector<int>& topo) {
  convMigrations.clear();
  if (!convMigrate) return;
  for (int id : topo) {
    if (nodes[id]->type != GA_NODE_CONVOLVER) continue;
    ConvolverS& nd = rec<ConvolverS>(*nodes[id]);
    if (!nd.ir || !nd.refSens || (nd.convPath != 4 && nd.convPath != 1)) continue;
    const int P = nd.ir->P;
    if (nd.convPath == 1) {
      // Formulation A keeps a spectra history and an overlap of the same meaning as B's, in the columns of its groups ([129 (P-1)][rp],
      // column idx; rows of a node = impulse-response channels = slots): a state copy.  A's spectra come from float32 transforms, so
      // the P - 1 blocks behind the move are R's arithmetic over A's spectra (inside the convolver tolerance), and one block later --
      // the overlap it reads is the first one made of R's spectra alone -- the output is that of a node on R from its first block.
      const int channels = nd.ir->nch, h = P - 1;
      if ((int)nd.convRows.size() != channels) continue;   // (rows not made yet: assignConvPaths decides)
      nd.bInCh = nd.isTrueStereo ? 2 : channels;
      nd.bSlots = nd.isTrueStereo ? 4 : channels;
      const size_t hstride = (size_t)kBins * std::max(h, 1);
      const size_t hb = (size_t)nd.bInCh * hstride * sizeof(float), ob = (size_t)nd.bSlots * 2 * kBlock * sizeof(float);
      nd.bHistR = (float*)dalloc(hb);
      nd.bHistI = (float*)dalloc(hb);
      nd.bOverlap = (float*)dalloc(ob);
      GA_HIP(hipMemsetAsync(nd.bHistR, 0, hb, stream));
      GA_HIP(hipMemsetAsync(nd.bHistI, 0, hb, stream));
      GA_HIP(hipMemsetAsync(nd.bOverlap, 0, ob, stream));
      bool any = false;
      for (int c = 0; c < nd.bInCh && h > 0; c++) {   // the row of a slot that reads input channel c
        const ConvRowRef& rr = nd.convRows[nd.isTrueStereo ? 2 * c : c];
        const ConvGroup& g = *rr.group;
        if (g.histZero || !g.histR) continue;
        GA_HIP(hipMemcpy2DAsync(nd.bHistR + c * hstride, 4, g.histR + rr.idx, (size_t)g.rp * 4, 4, (size_t)kBins * h, hipMemcpyDeviceToDevice, stream));
        GA_HIP(hipMemcpy2DAsync(nd.bHistI + c * hstride, 4, g.histI + rr.idx, (size_t)g.rp * 4, 4, (size_t)kBins * h, hipMemcpyDeviceToDevice, stream));
        any = true;
      }
      for (int slot = 0; slot < nd.bSlots && slot < (int)nd.convRows.size(); slot++) {
        const ConvRowRef& rr = nd.convRows[slot];
        ConvGroup& g = *rr.group;
        if (g.overlap[g.ovCur] && !g.histZero) {
          GA_HIP(hipMemcpyAsync(nd.bOverlap + (size_t)slot * 2 * kBlock, g.overlap[g.ovCur] + (size_t)rr.idx * kBlock, kBlock * 4, hipMemcpyDeviceToDevice, stream));
          any = true;
        }
        g.rows[rr.idx] = {-1, 0};   // (released as moveRows releases them)
      }
      nd.convRows.clear();
      nd.bShared = false;
      nd.bHistZero = !any;
      nd.bHistPlane = -1;
      nd.bOvCur = 0;
      nd.convPath = 2;   // (P <= 64, or no block-axis transforms: formulation A is never taken where C would be)
      stats.conv_migrations++;
      continue;
    }
    ConvMigration mg{};
    mg.id = id;
    const int nxr = nd.bShared ? 1 : nd.bInCh;   // (bInCh / bSlots / bShared carry over: both layouts define them alike)
    bool any = false;
    for (int ch = 0; ch < nxr && ch < 32; ch++) {
      const float* h = coarseHistory(nd, ch);
      mg.src[ch] = h ? h + conv_rebuild_src_offset(nd.dHistLen, P) : nullptr;
      any = any || h != nullptr;
    }
    const size_t hb = (size_t)nd.bInCh * kBins * std::max(P - 1, 1) * sizeof(float);
    const size_t ob = (size_t)nd.bSlots * 2 * kBlock * sizeof(float);
    nd.bHistR = (float*)dalloc(hb);
    nd.bHistI = (float*)dalloc(hb);
    nd.bOverlap = (float*)dalloc(ob);
    GA_HIP(hipMemsetAsync(nd.bHistR, 0, hb, stream));
    GA_HIP(hipMemsetAsync(nd.bHistI, 0, hb, stream));
    GA_HIP(hipMemsetAsync(nd.bOverlap, 0, ob, stream));
    nd.bHistZero = !any;   // (nothing in front of the chunk yet: an empty delay line, no launch)
    nd.bHistPlane = -1;
    nd.bOvCur = 0;
    nd.convPath = (useTimeFft && P > 64 && P <= 1024) ? 3 : 2;   // (the rule of assignConvPaths)
    for (int b = 0; b < 2; b++) {
      if (nd.dHistBase[b]) retired.push_back({nd.dHistBase[b], nd.dHistBytes});
      if (nd.dTail[b]) retired.push_back({nd.dTail[b], (size_t)nd.dTailLen * nd.dTailCh * sizeof(float)});
      nd.dHistBase[b] = nullptr;
      nd.dHist[b] = nd.dTail[b] = nullptr;
    }
    nd.dHistExt.clear();   // (a buffer it referred to is released behind a stream wait: Context::collectGarbage)
    nd.dHistBytes = 0;
    nd.dHistLen = 0;
    nd.dHistCur = 0;
    nd.dHistZero = true;
    nd.dTailLen = 0;
    nd.dTailCh = nd.dTailCur = 0;
    nd.dTailSig = 0;
    nd.dTailSeq = ~0ull - 1;
    nd.dLeader = -1;
    nd.dGroupSize = 0;
    fusionKeyValid = false;
    stats.conv_migrations++;
    if (any) convMigrations.push_back(mg);
  }
}

// The rebuild of every node that leaves formulation D in this chunk, in three launches whatever their number: conv_rebuild_kernel
// (job = input channel), then block T-1 alone through R's own partition sum and inverse transform on scratch planes -- an
// overlap-in of zeros (the overlap-add touches the first half only) and no output row; what it leaves is the overlap the chunk's
// first block reads.  Plan entries: ordered with the chunk's launches, no host wait.
void Context::planConvMigration(ChunkRun& r) {
  Exec& ex = *r.ex;
  const std::vector<ConvMigration> all = std::move(convMigrations);
  convMigrations.clear();
  std::vector<const ConvMigration*> mine;
  int maxP = 1;
  for (const ConvMigration& mg : all) {
    mine.push_back(&mg);
    maxP = std::max(maxP, rec<ConvolverS>(*nodes[mg.id]).ir->P);
  }
  const int hist = conv_rebuild_hist(maxP), tx = conv_rebuild_tx(maxP), ty = kRebuildTy;
  std::vector<ConvRebuildJob> jobs;
  std::vector<ConvSetB> sets;
  std::vector<ConvRowIO> yrows;
  std::vector<const float*> ovIn;
  std::vector<float*> ovOut;
  double flops = 0;
  for (const ConvMigration* mg : mine) {
    ConvolverS& nd = rec<ConvolverS>(*nodes[mg->id]);
    const int P = nd.ir->P;
    const size_t hstride = (size_t)kBins * std::max(P - 1, 1);
    const int nxr = nd.bShared ? 1 : nd.bInCh;
    const int x0 = (int)jobs.size();
    for (int ch = 0; ch < nxr; ch++) jobs.push_back(ConvRebuildJob{mg->src[ch], nd.bHistR + ch * hstride, nd.bHistI + ch * hstride, P, x0 + ch});
    conv_for_each_set(nd.bShared, nd.isTrueStereo, nxr, nd.bSlots, [&](int xc, const int* slots, int ncol) {
      sets.push_back(makeSetB(*nd.ir, x0 + xc, (int)yrows.size(), slots, ncol));
      for (int j = 0; j < ncol; j++) {   // no output row, an overlap-in of zeros: what is left is the overlap the chunk's first block reads
        yrows.push_back(ConvRowIO{nullptr, nullptr});
        ovIn.push_back(zeros);
        ovOut.push_back(nd.bOverlap + ((size_t)slots[j] * 2 + nd.bOvCur) * kBlock);
      }
    });
    flops += 8.0 * P * kBins * (double)nd.bSlots;
  }
  // scratch planes of this chunk alone: freed with the retire list, after the stream has run the launches below
  const size_t xb = jobs.size() * kBins * (size_t)tx * sizeof(float), yb = yrows.size() * kBins * (size_t)ty * sizeof(float);
  float* scratch = (float*)dalloc(2 * xb + 2 * yb);
  retired.push_back({scratch, 2 * xb + 2 * yb});
  ConvPlanesB plb{scratch, scratch + xb / sizeof(float), scratch + 2 * xb / sizeof(float), scratch + (2 * xb + yb) / sizeof(float), tx, ty};
  const size_t jo = ex.plan.putv(jobs), so = ex.plan.putv(sets), yo = ex.plan.putv(yrows), oi = ex.plan.putv(ovIn), oo = ex.plan.putv(ovOut);
  const int nj = (int)jobs.size(), ns_ = (int)sets.size(), ny = (int)yrows.size();
  hipStream_t st = stream;
  Twiddles tw = twiddles();
  Context* cp = this;
  ex.plan.add(LK_FFT, [=](uint8_t* base) {
    GA_HIP(hipMemsetAsync(scratch, 0, 2 * xb, st));   // (columns in front of a shorter node's first block)
    launch_conv_rebuild(st, (const ConvRebuildJob*)(base + jo), nj, maxP, plb, hist, tw);
    cp->noteKernel(LK_FFT, "conv_rebuild_kernel");
  });
  ex.plan.add(LK_MAC, [=](uint8_t* base) {
    launch_refmac(st, (const ConvSetB*)(base + so), ns_, 1, hist, plb);
    cp->noteKernel(LK_MAC, "refmac_kernel");
  }, 0.0, flops);
  ex.plan.add(LK_FFT, [=](uint8_t* base) {
    launch_irfft_ola_b(st, (const ConvRowIO*)(base + yo), ny, 1, plb, (const float* const*)(base + oi), (float* const*)(base + oo), tw, true);
  });
}

// pass 5: convolver formulations of new nodes, fusion groups, scratch arenas (sized before any recorded launch captures them)
void Context::chunkConvScratch(ChunkRun& r) {
  std::vector<int>& topo = r.topo;
  int64_t& n = r.n;
  int& bHistMax = r.bHistMax;
  // resampler trajectories used in this chunk go into one device table
  for (auto& kv : resamplers) kv.second->devOffset = -1;

  // ---- convolver scratch planes are shared by all groups: size them for the largest group BEFORE any recorded
  //      launch captures their address ----
  if (topology.hasConvolvers && r.stage != 1) {   // (no convolver in the first stage of a two-stage chunk: chunkTopology) (a graph without convolvers -- tens of thousands of nodes of config 4 -- skips these sweeps)
    refOrderSensitivity(topo);
    migrateConvolvers(topo);   // (option "conv_migrate": before the paths, the fusion groups and the scratch sizes are decided)
    assignConvPaths(topo, n);
    for (int id : topo) {
      if (nodes[id]->type != GA_NODE_CONVOLVER) continue;
      ConvolverS& nd = rec<ConvolverS>(*nodes[id]);
      nd.refOrder = nd.refSens && nd.ir && (nd.convPath == 2 || nd.convPath == 3);
    }
    planCoarseFusion(topo, r.segs);
    for (int id : topo)
      if (nodes[id]->type == GA_NODE_CONVOLVER) rec<ConvolverS>(*nodes[id]).dGroupSize = 0;
    for (int id : topo) {
      if (nodes[id]->type != GA_NODE_CONVOLVER) continue;
      const ConvolverS& nd = rec<ConvolverS>(*nodes[id]);
      if (nd.ir && nd.convPath == 4 && nd.dLeader >= 0) rec<ConvolverS>(*nodes[nd.dLeader]).dGroupSize++;
    }
    aliasBusToLeader(r);
  }
  bHistMax = 0;
  if (topology.hasConvolvers) {
    size_t xMax = 0, yMax = 0;
    size_t bx = 0, by = 0;
    for (int id : topo) {
      if (nodes[id]->type != GA_NODE_CONVOLVER) continue;
      ConvolverS& nd = rec<ConvolverS>(*nodes[id]);
      if (!nd.ir) continue;
      if (nd.convPath == 2 || nd.convPath == 3) {
        bx += nd.bInCh;
        by += nd.bSlots;
        bHistMax = std::max(bHistMax, nd.ir->P - 1);
      }
      for (auto& rr : nd.convRows) {
        ConvGroup& g = *rr.group;
        ensureGroupState(g);
        const int ty_ = (int)roundup(n, 64), tx_ = ty_ + g.P + 128;
        xMax = std::max(xMax, (size_t)kBins * tx_ * g.rp * sizeof(float));
        yMax = std::max(yMax, (size_t)kBins * ty_ * g.rp * sizeof(float));
      }
    }
    if (xMax) {
      ensure(planes[0], xMax);
      ensure(planes[1], xMax);
      ensure(planes[2], yMax);
      ensure(planes[3], yMax);
    }
    {  // formulation D: the stages of a chunk run one after the other on the stream and share the two arenas
      std::map<int, std::pair<size_t, size_t>> perDepth;   // depth -> (X frames, Y rows upper bound)
      std::map<int, int> tailDepth;                        // depth -> longest carried tail a group of the stage can have (coarse blocks)
      const int64_t nT = (n * kBlock + kCoarseBlock - 1) / kCoarseBlock;
      for (int id : topo) {
        if (nodes[id]->type != GA_NODE_CONVOLVER) continue;
        ConvolverS& nd = rec<ConvolverS>(*nodes[id]);
        if (!nd.ir || nd.convPath != 4) continue;
        auto& pd = perDepth[nd.depth];
        pd.first += (size_t)nd.bInCh * (size_t)(nT + nd.ir->coarseP);   // (+ the window behind the chunk's last block: carried tails)
        // Y rows: one per slot unless fused; fused groups need (members / 32 + 1) x channels rows, never more than the slots
        // Every Y row of a stage is nT + (the longest carried tail of the stage) frames long (CoarseStage::buildOutputs): ONE long group
        // stretches the rows of every convolver at its depth, so the rows are counted per depth and multiplied by the depth's row length
        pd.second += (size_t)nd.bSlots;
        int& tp = tailDepth[nd.depth];
        tp = std::max(tp, std::max(kCoarseMaxP, nd.ir->coarseP));
      }
      size_t xf = 0, yf = 0;
      for (auto& kv : perDepth) {
        xf = std::max(xf, kv.second.first);
        yf = std::max(yf, kv.second.second * (size_t)(nT + tailDepth[kv.first]));
      }
      if (xf) {
        ensure(coarseX, xf * kCoarseBins * sizeof(float2));
        ensure(coarseY, yf * kCoarseBins * sizeof(float2));
      }
      if (coarsePremix) {   // pre-mixed groups: [history | chunk] of the mixed signal per input channel of the group
        std::map<int, int> members;
        for (int id : topo) {
          if (nodes[id]->type != GA_NODE_CONVOLVER) continue;
          const ConvolverS& nd = rec<ConvolverS>(*nodes[id]);
          if (nd.ir && nd.convPath == 4) members[nd.dLeader >= 0 ? nd.dLeader : id]++;
        }
        std::map<int, size_t> pmDepth;
        for (auto& kv : members) {
          if (kv.second < 2) continue;
          const ConvolverS& ld = rec<ConvolverS>(*nodes[kv.first]);
          pmDepth[ld.depth] += (size_t)ld.bInCh * ((((size_t)(ld.dHistLen + n * kBlock) * sizeof(float)) + 255) & ~(size_t)255);
        }
        size_t pm = 0;
        for (auto& kv : pmDepth) pm = std::max(pm, kv.second);
        if (pm) ensure(coarseM, 2 * pm + 512);   // (two halves, used in turn)
      }
    }
    bRowX = bRowY = 0;
    if (bx) {  // formulation B scratch: [row][bin][block]; x planes alternate between two pairs (flushPlaneHistories)
      const size_t txb = (size_t)roundup(bHistMax, 4) + roundup(n, 16) + 16, tyb = (size_t)roundup(n, 256);
      bPairWrite = bPairCur ^ 1;
      flushPlaneHistories(bPairWrite);
      // both pairs grow together (a render that continues reaches the other pair in its next chunk; growing it then would
      // put an allocation into the steady state), but only a pair without residents can be reallocated
      const size_t xb = bx * kBins * txb * sizeof(float);
      if (planesB[0].bytes < xb || planesBalt[0].bytes < xb) flushPlaneHistories(bPairCur);
      ensure(planesB[0], xb);
      ensure(planesB[1], xb);
      ensure(planesBalt[0], xb);
      ensure(planesBalt[1], xb);
      ensure(planesB[2], by * kBins * tyb * sizeof(float));
      ensure(planesB[3], by * kBins * tyb * sizeof(float));
    }
  }

  if (topology.hasOscillators)
  for (int id : topo) {  // OscillatorNode._phase lives on the device (one double, zero at Start)
    if (nodes[id]->type != GA_NODE_OSCILLATOR) continue;
    OscillatorS& nd = rec<OscillatorS>(*nodes[id]);
    if (nd.oscPhase) continue;
    nd.oscPhase = (double*)dalloc(64);
    GA_HIP(hipMemsetAsync(nd.oscPhase, 0, 64, stream));
  }
}

// formulation A: convolvers that share an impulse-response channel run as one group per (impulse response, channel) -- the
// banded-Toeplitz matrix-core kernel or the block-axis transforms over all their rows (PartitionedConvolver.cs:104-223)
void Context::planConvolversShared(ChunkRun& r, ConvPlanCtx& k) {
  const int64_t n = r.n;
  Exec& ex = *r.ex;
  std::vector<const float*> prevIns;   // the inputs of the group planned before this one (forward spectra still in the scratch planes)
  int prevP = -1, prevRp = -1, prevRows = -1;
  for (auto& kv : k.active) {
    ConvGroup& g = *kv.first;
    const int P = g.P, hist = P - 1;
    const int nrows = (int)g.rows.size();
    std::vector<ConvRowIO> rio(nrows, ConvRowIO{nullptr, nullptr});
    for (auto& ns_ : kv.second) {
      ConvolverS& nd = rec<ConvolverS>(*nodes[ns_.first]);
      const int slot = ns_.second;
      // which input channel feeds this row: discrete -> slot ; true stereo -> L,L,R,R for h0,h1,h2,h3 (ConvolverNode.cs:127-151)
      const float* in = convChunkInput(*this, ex, ex.convIn[ns_.first], conv_slot_input(nd.isTrueStereo, slot));
      // (true stereo: temp1 / temp2, summed behind the stage, ConvolverNode.cs:137-143)
      float* out = nd.isTrueStereo ? trueStereoTemp(*this, k, ns_.first, slot) : ex.nodeOut(ns_.first, slot);
      rio[nd.convRows[slot].idx] = ConvRowIO{in, out};
    }
    ex.flushLevel();
    const int rp = g.rp;
    const int ty = (int)roundup(n, 64);
    const int tx = ty + P + 128;
    ConvPlanes pl{(float*)planes[0].p, (float*)planes[1].p, (float*)planes[2].p, (float*)planes[3].p, tx, ty, rp};
    size_t rioOff = ex.plan.putv(rio);
    hipStream_t st = stream;
    Twiddles tw = twiddles();
    const int nn = (int)n;
    float* hR = g.histR;
    float* hI = g.histI;
    const bool hz = g.histZero;
    const float* hr = g.ir->hr + (size_t)g.irCh * kBins * P;
    const float* hi = g.ir->hi + (size_t)g.irCh * kBins * P;
    float* ovIn = g.overlap[g.ovCur];
    float* ovOut = g.overlap[g.ovCur ^ 1];
    g.ovCur ^= 1;
    g.histZero = false;
    // forward spectra depend only on the inputs: a group fed by exactly the same signals as the previous one (e.g. the
    // channels of one stereo IR behind mono voices) reuses the X rows that are still in the scratch planes
    std::vector<const float*> ins(nrows);
    for (int r = 0; r < nrows; r++) ins[r] = rio[r].in;
    const bool skipFwd = (prevP == P && prevRp == rp && prevRows == nrows && prevIns == ins);
    prevIns = ins;
    prevP = P;
    prevRp = rp;
    prevRows = nrows;
    ex.plan.add(LK_FFT, [=](uint8_t* base) {
      // frequency-domain delay line of the previous chunk(s) in front of this chunk's spectra
      if (hist > 0) {
        launch_plane_copy(st, pl.xr, tx, 0, hz ? nullptr : hR, hist, 0, hist, rp);
        launch_plane_copy(st, pl.xi, tx, 0, hz ? nullptr : hI, hist, 0, hist, rp);
      }
      // rows beyond this chunk that the banded MAC may touch for its (discarded) padded outputs
      int tail = std::min(tx - (hist + nn), 256);
      launch_plane_copy(st, pl.xr, tx, hist + nn, nullptr, 0, 0, tail, rp);
      launch_plane_copy(st, pl.xi, tx, hist + nn, nullptr, 0, 0, tail, rp);
      if (!skipFwd) launch_rfft_fwd(st, (const ConvRowIO*)(base + rioOff), nrows, nn, hist, pl, tw);
    });
    ex.plan.add(LK_MAC, [=](uint8_t*) { launch_spectral_mac_shared(st, pl, hr, hi, P, nn, nrows); });
    ex.plan.add(LK_FFT, [=](uint8_t* base) {
      launch_irfft_ola(st, (const ConvRowIO*)(base + rioOff), nrows, nn, pl, ovIn, ovOut, tw);
      if (hist > 0) {  // keep the last P-1 spectra for the next chunk (the FDL, PartitionedConvolver.cs:122-128)
        launch_plane_copy(st, hR, hist, 0, pl.xr, tx, nn, hist, rp);
        launch_plane_copy(st, hI, hist, 0, pl.xi, tx, nn, hist, rp);
      }
    });
    stats.mac_flops_total += 8.0 * P * kBins * (double)kv.second.size() * (double)n;
    // streaming-formulation bytes: per channel-instance per block FDL read + write + input, IR once per block per channel
    stats.mac_bytes_total += ((double)P * kBins * 8.0 + kBins * 8.0 + 512.0) * (double)kv.second.size() * (double)n +
                             (double)P * kBins * 8.0 * (double)n;
    stats.mac_launches += 1;
  }
}

// One private-IR convolver stage of a chunk: nodes with an impulse response of their own on the B / C state layout (per-node planes;
// the direct partition sum, block-axis FFT segments, or -- refOrder -- formulation R: the reference's own order between
// double-precision transforms).  Planned node by node in four passes, then enqueued and accounted (planPrivateStage).
namespace {
struct PrivateStage {
  Context& c;
  Exec& ex;
  ConvPlanCtx& k;
  const std::vector<int>& bNodes;
  const bool refOrder;
  const int64_t n;
  const int hist;       // plane time origin, 16-byte aligned rows
  const int txb, tyb;   // columns of an x row / a y row
  // rows of this stage start after the rows of the stages before it: a node's spectra stay intact for the next chunk
  const size_t rowX0, rowY0;
  const ConvPlanesB plb;
  struct SetTaps { IrSpectra* ir; int slot[kConvSetCols]; };
  using TconvLaunch = Context::TconvLaunch;
  std::vector<ConvRowIO> xrows, yrows;
  std::vector<HistJobB> restore;
  std::vector<ConvSetB> sets;                        // formulations B and R
  std::map<int, std::vector<ConvSetC>> setsC;        // formulation C, by P: launches per distinct segment length
  std::map<int, std::vector<SetTaps>> setsCTaps;     // which taps spectra each column of a set needs (filled per FFT length)
  std::vector<const float*> ovIn;
  std::vector<float*> ovOut;
  double flops = 0;
  Views chIn;   // chunk-long views of the current node's input channels

  PrivateStage(Context& c_, ChunkRun& r, ConvPlanCtx& k_, const std::vector<int>& nodes_, bool refOrder_)
      : c(c_), ex(*r.ex), k(k_), bNodes(nodes_), refOrder(refOrder_), n(r.n), hist((int)roundup(r.bHistMax, 4)),
        txb(hist + (int)roundup(r.n, 16) + 16), tyb((int)roundup(r.n, 256)), rowX0(c_.bRowX), rowY0(c_.bRowY),
        plb{c_.xPlane(c_.bPairWrite, 0) + rowX0 * kBins * txb, c_.xPlane(c_.bPairWrite, 1) + rowX0 * kBins * txb,
            (float*)c_.planesB[2].p + rowY0 * kBins * tyb, (float*)c_.planesB[3].p + rowY0 * kBins * tyb, txb, tyb} {}
  void resolveInputs(int id, ConvolverS& nd);          // chunk-long input views; the shared -> private history hand-down
  int buildRows(ConvolverS& nd);                       // x rows and the jobs that restore their columns around the chunk; -> first row
  void buildSets(int id, ConvolverS& nd, int x0);      // B / R sets, C sets and their tap lists, y rows, overlaps
  void keepHistory(int id, ConvolverS& nd, int x0);    // where the next chunk finds this node's last P - 1 spectra
  void enqueue();                                      // tables into the plan, launches
  void enqueueTimeFft();                               // formulation C: one launch per P and segment length
  void account();                                      // flops, streaming-formulation bytes, the stage's launch count
};

void PrivateStage::resolveInputs(int id, ConvolverS& nd) {
  chIn.assign(nd.bInCh, nullptr);
  for (int ch = 0; ch < nd.bInCh; ch++) chIn[ch] = convChunkInput(c, ex, ex.convIn[id], ch);
  bool allSame = true;
  for (int ch = 1; ch < nd.bInCh; ch++) allSame = allSame && (chIn[ch] == chIn[0]);
  if (!nd.bShared || allSame) return;
  // the channels start to differ: every channel inherits the (so far common) history of channel 0
  const int h = nd.ir->P - 1;
  const size_t hstride = (size_t)kBins * std::max(h, 1);
  if (!nd.bHistZero && h > 0 && nd.bHistPlane < 0)   // (a plane-resident shared row is simply read by every channel)
    for (int ch = 1; ch < nd.bInCh; ch++) {   // (plan entries: ordered with the chunk's launches)
      float *dr = nd.bHistR + ch * hstride, *di = nd.bHistI + ch * hstride;
      const float *sr = nd.bHistR, *sim = nd.bHistI;
      hipStream_t st = c.stream;
      ex.plan.add(LK_OTHER, [dr, di, sr, sim, hstride, st](uint8_t*) {
        GA_HIP(hipMemcpyAsync(dr, sr, hstride * 4, hipMemcpyDeviceToDevice, st));
        GA_HIP(hipMemcpyAsync(di, sim, hstride * 4, hipMemcpyDeviceToDevice, st));
      });
    }
  nd.bShared = false;
}

int PrivateStage::buildRows(ConvolverS& nd) {
  const int h = nd.ir->P - 1;
  const size_t hstride = (size_t)kBins * std::max(h, 1);
  const int nxr = nd.bShared ? 1 : nd.bInCh;
  const int x0 = (int)xrows.size();
  for (int ch = 0; ch < nxr; ch++) {
    const int xi = x0 + ch;
    xrows.push_back(ConvRowIO{chIn[ch], nullptr});
    float* xr_row = plb.xr + (size_t)xi * kBins * txb;
    float* xi_row = plb.xi + (size_t)xi * kBins * txb;
    // [0, hist - h) zeros, [hist - h, hist) this channel's history, rows after the chunk zero (K padding reads them)
    if (hist - h > 0) {
      restore.push_back(HistJobB{xr_row, nullptr, txb, 0, hist - h, 0});
      restore.push_back(HistJobB{xi_row, nullptr, txb, 0, hist - h, 0});
    }
    if (h > 0) {
      const float *srcR = nullptr, *srcI = nullptr;
      int sstride = h;
      if (nd.bHistZero) {
      } else if (nd.bHistPlane >= 0) {   // the previous chunk's x planes (never the pair being written: flushed in chunkConvScratch)
        const size_t off = (size_t)(nd.bHistRow + (nd.bHistNx == 1 ? 0 : ch)) * kBins * nd.bHistTxb + nd.bHistOff;
        srcR = c.xPlane(nd.bHistPlane, 0) + off;
        srcI = c.xPlane(nd.bHistPlane, 1) + off;
        sstride = nd.bHistTxb;
      } else {
        srcR = nd.bHistR + ch * hstride;
        srcI = nd.bHistI + ch * hstride;
      }
      restore.push_back(HistJobB{xr_row + (hist - h), srcR, txb, sstride, h, 0});
      restore.push_back(HistJobB{xi_row + (hist - h), srcI, txb, sstride, h, 0});
    }
    const int tailn = txb - (hist + (int)n);
    restore.push_back(HistJobB{xr_row + hist + (int)n, nullptr, txb, 0, tailn, 0});
    restore.push_back(HistJobB{xi_row + hist + (int)n, nullptr, txb, 0, tailn, 0});
  }
  return x0;
}

void PrivateStage::buildSets(int id, ConvolverS& nd, int x0) {
  // slots: discrete -> slot c reads input c, IR channel c ; true stereo -> (L,h0) (L,h1) (R,h2) (R,h3), into temps summed behind the stage
  float* slotOut[32];
  if (nd.bSlots > 32) fail(GA_ERR_INVALID_OPERATION, "internal: more than 32 convolver slots");
  for (int slot = 0; slot < nd.bSlots; slot++) slotOut[slot] = nd.isTrueStereo ? trueStereoTemp(c, k, id, slot) : ex.nodeOut(id, slot);
  const int P = nd.ir->P;
  conv_for_each_set(nd.bShared, nd.isTrueStereo, nd.bShared ? 1 : nd.bInCh, nd.bSlots, [&](int xc, const int* slots, int ncol) {
    const int y0 = (int)yrows.size();
    for (int j = 0; j < ncol; j++) {   // y rows consecutive per set
      yrows.push_back(ConvRowIO{nullptr, slotOut[slots[j]]});
      ovIn.push_back(nd.bOverlap + ((size_t)slots[j] * 2 + nd.bOvCur) * kBlock);
      ovOut.push_back(nd.bOverlap + ((size_t)slots[j] * 2 + (nd.bOvCur ^ 1)) * kBlock);
    }
    if (refOrder || nd.convPath != 3) {
      sets.push_back(makeSetB(*nd.ir, x0 + xc, y0, slots, ncol));
      if (refOrder) c.stats.ref_order_rows += ncol;
    } else {
      ConvSetC sc{};   // (hs: per FFT length, enqueueTimeFft)
      sc.x = x0 + xc;
      sc.y0 = y0;
      sc.ncol = ncol;
      sc.P = P;
      SetTaps tp{nd.ir.get(), {}};
      std::copy(slots, slots + ncol, tp.slot);
      setsC[P].push_back(sc);
      setsCTaps[P].push_back(tp);
    }
  });
  nd.bOvCur ^= 1;
  flops += 8.0 * P * kBins * (double)nd.bSlots * (double)n;
}

void PrivateStage::keepHistory(int id, ConvolverS& nd, int x0) {
  const int h = nd.ir->P - 1;
  nd.bHistZero = false;
  if (h == 0) return;
  // the history of the next chunk: the last h spectra of this node's rows, read where they lie
  if (nd.bHistPlane == c.bPairWrite) fail(GA_ERR_DEVICE, "internal: convolver history lives in the planes being written");
  nd.bHistPlane = c.bPairWrite;
  nd.bHistRow = (int)rowX0 + x0;
  nd.bHistNx = nd.bShared ? 1 : nd.bInCh;
  nd.bHistOff = hist + (int)n - h;
  nd.bHistTxb = txb;
  c.bResidents[c.bPairWrite].push_back(id);
}

void PrivateStage::enqueue() {
  c.bRowX += xrows.size();   // (the next stage's rows lie behind these)
  c.bRowY += yrows.size();
  c.bPairCur = c.bPairWrite;
  ex.flushLevel();   // (materialised inputs)
  // (the launches below run after this object is gone: they capture what they name, never members)
  const size_t xo = ex.plan.putv(xrows), yo = ex.plan.putv(yrows), so = ex.plan.putv(sets), ro = ex.plan.putv(restore),
               oi = ex.plan.putv(ovIn), oo = ex.plan.putv(ovOut);
  const int nx = (int)xrows.size(), ny = (int)yrows.size(), ns_ = (int)sets.size(), nr = (int)restore.size();
  const int nn = (int)n, hist = this->hist;
  const int maxn = std::max(hist, txb - hist - nn);
  const ConvPlanesB plb = this->plb;
  const bool ref = refOrder;
  const bool f64 = c.fft64 || ref;   // (formulation R: the reference's FftFlat precision around its own partition sum)
  const double flops = this->flops;
  hipStream_t st = c.stream;
  const Twiddles tw = c.twiddles();
  Context* cp = &c;
  ex.plan.add(LK_FFT, [st, ro, nr, maxn, xo, nx, nn, hist, plb, tw, f64](uint8_t* base) {
    launch_hist_copy_b(st, (const HistJobB*)(base + ro), nr, std::max(maxn, 1));
    launch_rfft_fwd_b(st, (const ConvRowIO*)(base + xo), nx, nn, hist, plb, tw, f64);
  });
  // (formulation R: 8 separately rounded operations per complex multiply-add -- the planner's count of what the launch executes)
  if (ns_ > 0)
    ex.plan.add(LK_MAC, [st, so, ns_, nn, hist, plb, ref, cp](uint8_t* base) {
      if (ref) launch_refmac(st, (const ConvSetB*)(base + so), ns_, nn, hist, plb);
      else launch_spectral_mac_b(st, (const ConvSetB*)(base + so), ns_, nn, hist, plb);
      cp->noteKernel(LK_MAC, ref ? "refmac_kernel" : "spectral_mac_b_kernel");
    }, 0.0, flops);
  enqueueTimeFft();
  ex.plan.add(LK_FFT, [st, yo, ny, nn, plb, oi, oo, tw, f64](uint8_t* base) {
    launch_irfft_ola_b(st, (const ConvRowIO*)(base + yo), ny, nn, plb, (const float* const*)(base + oi), (float* const*)(base + oo), tw, f64);
  });
}

void PrivateStage::enqueueTimeFft() {
  const int nn = (int)n, hist = this->hist;
  const ConvPlanesB plb = this->plb;
  hipStream_t st = c.stream;
  for (auto& kv : setsC) {
    const int Pc = kv.first;
    static const char* r16env = expenv("GA_TCONV_RADIX16");   // A/B switches for measurements
    static const char* planenv = expenv("GA_TCONV_MIXED");
    const bool r16 = r16env ? atoi(r16env) != 0 : c.useRadix16;
    std::vector<TconvLaunch> tplan;
    if (c.debugTconvN2 > 0) {   // tests: a length no kernel exists for must come back as an error code, not abort the host
      const int Lc = std::max(1, c.debugTconvN2 - (Pc - 1));
      tplan.push_back(TconvLaunch{c.debugTconvN2, 0, (nn + Lc - 1) / Lc});
    } else if (r16 && !(planenv && atoi(planenv) == 0)) {
      tplan = c.tconvPlan(nn, Pc);
    } else {   // one FFT length for the whole chunk
      const int N2 = tapFftSize(Pc), Lc = N2 - (Pc - 1);
      tplan.push_back(TconvLaunch{N2, 0, (nn + Lc - 1) / Lc});
    }
    const std::vector<SetTaps>& taps = setsCTaps[Pc];
    for (const TconvLaunch& tl : tplan) {
      std::vector<ConvSetC> sv = kv.second;
      for (size_t i = 0; i < sv.size(); i++) {
        const float2* hsp = c.ensureTapSpectra(*taps[i].ir, tl.N2);
        for (int j = 0; j < sv[i].ncol; j++) sv[i].hs[j] = hsp + (size_t)taps[i].slot[j] * kBins * tl.N2;
      }
      const size_t co = ex.plan.putv(sv);
      const int nc = (int)sv.size();
      const int N2 = tl.N2, tbase = tl.tbase, nseg = tl.nseg;
      const float2* twc = r16 ? c.twiddles16(N2) : c.twiddlesC(N2);
      ex.plan.add(LK_MAC, [st, co, nc, nn, hist, plb, N2, twc, nseg, tbase, r16](uint8_t* base) {
        if (r16) launch_tconv16(st, (const ConvSetC*)(base + co), nc, nn, hist, plb, N2, twc, nseg, tbase);
        else launch_tconv(st, (const ConvSetC*)(base + co), nc, nn, hist, plb, N2, twc, nseg);
      });
    }
  }
}

void PrivateStage::account() {
  c.stats.mac_flops_total += flops;
  // streaming-formulation bytes: per channel-instance per block FDL read + write + input; every distinct
  // IR channel is counted once per block however many nodes share it
  std::map<std::pair<IrSpectra*, int>, int> distinct;
  double bytes = 0;
  for (int id : bNodes) {
    ConvolverS& nd = rec<ConvolverS>(*c.nodes[id]);
    const int P = nd.ir->P;
    bytes += ((double)P * kBins * 8.0 + kBins * 8.0 + 512.0) * nd.bSlots * (double)n;
    for (int sl = 0; sl < nd.bSlots; sl++) distinct[{nd.ir.get(), sl}] = P;
  }
  for (auto& kv : distinct) bytes += (double)kv.second * kBins * 8.0 * (double)n;
  c.stats.mac_bytes_total += bytes;
  c.stats.mac_launches += 1;
}
}  // namespace

static void planPrivateStage(Context& c, ChunkRun& r, ConvPlanCtx& k, const std::vector<int>& bNodes, bool refOrder) {
  PrivateStage s(c, r, k, bNodes, refOrder);
  for (int id : bNodes) {   // node by node: the order of slabs, terms and mix jobs decides the plan tables
    ConvolverS& nd = rec<ConvolverS>(*c.nodes[id]);
    s.resolveInputs(id, nd);
    const int x0 = s.buildRows(nd);
    s.buildSets(id, nd, x0);
    s.keepHistory(id, nd, x0);
  }
  s.enqueue();
  s.account();
}

// pass 7 (per convolver depth d): the convolvers whose inputs are complete, once per chunk over all blocks
void Context::chunkPlanConvolvers(ChunkRun& r, int d) {
  Exec& ex = *r.ex;
  // ---- convolvers whose inputs are complete (depth d): once per chunk over all blocks ----
  // group -> (node, slot); ordered by (IR buffer, IR channel) so groups fed by the same inputs are adjacent
  // (option "conv_migrate": the state of the nodes that left formulation D in this chunk is a function of earlier chunks' input alone --
  // rebuilt in front of the first convolver stage, for every depth at once)
  if (!convMigrations.empty()) planConvMigration(r);
  ConvPlanCtx k;
  std::vector<int> dNodes;        // formulation D nodes of this depth
  std::vector<int> plain, ref;    // formulation B / C nodes of this depth; those evaluated in the reference's order (formulation R)
  for (int id : r.topo) {
    if (nodes[id]->type != GA_NODE_CONVOLVER) continue;
    ConvolverS& nd = rec<ConvolverS>(*nodes[id]);
    if (!nd.ir || nd.depth != d) continue;
    if (!ex.convIn.has(id)) continue;
    if (nd.convPath == 4) {
      dNodes.push_back(id);
      continue;
    }
    if (nd.convPath >= 2) {
      (nd.refOrder ? ref : plain).push_back(id);
      continue;
    }
    for (int slot = 0; slot < (int)nd.convRows.size(); slot++) k.active[nd.convRows[slot].group].push_back({id, slot});
  }
  if (!k.active.empty()) planConvolversShared(r, k);
  // ---- formulation D: coarse partitions, consumer sums fused in the frequency domain ----
  if (!dNodes.empty()) planCoarseStage(*this, ex, dNodes, r.n);
  // ---- formulations B / C: nodes with a private impulse response ----
  // (those that this chunk evaluates in the reference's own order -- formulation R -- in a stage of their own: double-precision
  // transforms and launch_refmac instead of the matrix-core / block-axis-FFT partition sums)
  if (!plain.empty()) planPrivateStage(*this, r, k, plain, false);
  if (!ref.empty()) planPrivateStage(*this, r, k, ref, true);
  // true stereo: outL = conv0(L) + conv2(R) ; outR = conv1(L) + conv3(R)  (ConvolverNode.cs:127-144)
  for (auto& kv : k.tsTemps) {
    hipStream_t st = stream;
    int64_t fr = r.n * kBlock;
    for (int o = 0; o < 2; o++) {
      float* out = ex.nodeOut(kv.first, o);
      float *a = kv.second[o], *b2 = kv.second[o + 2];
      if (a && b2) ex.plan.add(LK_OTHER, [=](uint8_t*) { launch_pair_sum(st, out, a, b2, fr); });
    }
  }
}

}  // namespace ga
