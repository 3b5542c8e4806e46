// ga_topology.cpp -- the graph analysis of a chunk (ga_topology.hpp).  No HIP call and no Context member: the file compiles with the
// host compiler alone (tests/test_topology_host.py).  Which function decides what: DESIGN.md section 2c.
#include "ga_engine.hpp"

#include <cstdio>

namespace ga {
namespace {

// Everything a node pulls, in the order the reference pulls it: the modulation sources of every parameter, then the connections of
// every input (Nodes/AudioNode.cs:167-175).  Every walk of this file goes through here.
template <class F>
inline void forEachUpstream(const NodeS& nd, F&& f) {
  for (const ParamS& p : nd.params)
    for (const auto& m : p.modulation) f(m.first);
  for (const InputS& in : nd.inputs)
    for (const Conn& cn : in.connected) f(cn.node);
}

// a source whose playbackRate a signal modulates
inline bool rateModulated(const NodeS& nd) {
  return (nd.type == GA_NODE_BUFFER_SOURCE || nd.type == GA_NODE_STREAM_SOURCE) && !nd.params.empty() && !nd.params[0].modulation.empty();
}

// What, in the cone of a DelayNode, keeps that delay on the prediction (nullptr: nothing): an undecided DelayNode (the control state of
// the nodes in between would be undecided: more than two stages), a ConvolverNode (stage 1 plans no convolvers: their fusion groups and
// scratch planes belong to one pass over the whole graph), a source with a modulated playbackRate (stage 1 plans both from the state
// before the chunk).
inline const char* acceptanceBlocker(const NodeS& u) {
  if (u.type == GA_NODE_DELAY && !rec<DelayS>(u).delayAudible) return "another delay with its flag down";
  if (u.type == GA_NODE_CONVOLVER) return "a convolver";
  if (rateModulated(u)) return "a modulated rate";
  return nullptr;
}

// (experiment builds, GA_DEBUG_DELAY_FLAG: which condition keeps a delay on the prediction, one line per delay and chunk on stderr)
// (the reason is `why`, or `why` `what` `tail` where acceptanceBlocker names what)
inline void kept(const Topology& t, int id, int at, const char* why, const char* what = "", const char* tail = "") {
#ifdef GA_EXPERIMENTS
  if (expenv("GA_DEBUG_DELAY_FLAG"))
    fprintf(stderr, "[delay flag] chunk %lld delay %d keeps the prediction: %s%s%s (node %d)\n", (long long)t.chunkNo, id, why, what, tail, at);
#else
  (void)t, (void)id, (void)at, (void)why, (void)what, (void)tail;
#endif
}

// whole blocks of delay of a DelayNode whose delay is a constant (0: anything else)
int splittable(const NodeS& d, int sampleRate) {
  if (d.type != GA_NODE_DELAY || !d.params[0].events.empty() || !d.params[0].modulation.empty()) return 0;
  int dl = (int)(d.params[0].value * (float)sampleRate);   // DelayNode.cs:66 (float * int -> float, truncated)
  dl = std::min(std::max(dl, 0), rec<DelayS>(d).maxDelaySamples);
  return dl / kBlock;
}

// An upper estimate of the gain of the loop whose nodes are loop[n-1] .. loop[0] (the walk's stack from the node that closes it up): what a
// last-bit difference that enters it is multiplied by per turn.
double loopGain(const NodeTable& nodes, const int* loop, size_t n) {
  double bound = 1.0;
  for (size_t q = n; q-- > 0;) {
    const NodeS& mn = *nodes[loop[q]];
    bool moving = false;
    for (const ParamS& p : mn.params) moving = moving || !p.events.empty() || !p.modulation.empty();
    switch (mn.type) {
      case GA_NODE_GAIN: bound *= moving ? 1e9 : std::fabs((double)mn.params[0].value); break;
      case GA_NODE_BIQUAD: {
        const int ft = rec<BiquadS>(mn).filterType;
        if (moving) bound *= 1e9;
        else if (ft == GA_FILTER_PEAKING || ft == GA_FILTER_LOWSHELF || ft == GA_FILTER_HIGHSHELF)
          bound *= std::max(1.0, std::pow(10.0, (double)mn.params[2].value / 20.0));
        else bound *= std::max(1.0, (double)mn.params[1].value);   // (the resonance peak of a low / high / band pass is ~Q)
        break;
      }
      case GA_NODE_CONVOLVER: bound *= rec<ConvolverS>(mn).normalize ? 2.0 : 1e9; break;   // (normalised responses: broadband gain well below 1, peaks unknown)
      case GA_NODE_STEREO_PANNER: bound *= 2.0; break;                    // (oL = inL + inR * gainL)
      case GA_NODE_SPATIAL_PANNER: bound *= (double)rec<SpatialPannerS>(mn).spGainBound; break;   // (sum |F| + |D| <= max(1, sum |h|): g <= 1, the weights sum to 1)
      case GA_NODE_DYNAMICS_COMPRESSOR:   // (g = 10^((M - yL) / 20) with yL >= 0 to rounding: at most the makeup gain)
        bound *= moving ? 100.0 : std::max(1.0, std::pow(10.0, (double)std::min(std::max(mn.params[GA_COMPRESSOR_MAKEUP_GAIN].value, -40.f), 40.f) / 20.0));
        break;
      default: break;
    }
  }
  return bound;
}

// The walk from the destination, in the reference's order.  A node met again while it is still being processed closes a feedback
// cycle.  The reference does not refuse that: its memo check (Nodes/AudioNode.cs:153-156) returns before the "cycle detected" test can
// fire, and the consumer mixes the producer's PREVIOUS block.  Such an edge carries no ordering constraint -- the producer is processed
// later in the block, as there.
struct DestinationWalk {
  NodeTable& nodes;
  Topology& t;
  const TopologyOptions& o;
  std::vector<int>& order;
  std::vector<int> color, stack;
  std::vector<std::pair<int, int>> entry;   // (node, the node it was reached from) in the order the walk enters them
  std::vector<char> candidate;              // DelayNodes on a loop whose delay is a constant of at least two blocks
  bool unbreakable = false;                 // some loop holds no such DelayNode

  // the edge stack.back() -> id reads the block `id` put out last: it closes the loop of the stack's nodes from `id` up
  void closeLoop(int id) {
    if (o.delayFlagExact >= 2 && !stack.empty()) t.staleEdges.push_back(((uint64_t)stack.back() << 32) | (uint64_t)id);
    if (!nodes[id]->staleProducer) t.staleProducers.push_back(id);
    nodes[id]->staleProducer = true;
    if (candidate.empty()) candidate.assign(nodes.size(), 0);
    bool any = false;
    size_t first = stack.size();
    while (first > 0) {
      const int m = stack[--first];
      NodeS& mn = *nodes[m];
      if (mn.type == GA_NODE_DELAY) rec<DelayS>(mn).delayOnLoop = true;   // (option "delay_flag_exact")
      if (splittable(mn, o.sampleRate) >= 2) {   // it can be cut where a DelayNode delays by >= 2 blocks
        candidate[m] = 1;
        any = true;
      }
      if (m == id) break;
    }
    t.loopGainBound = std::max(t.loopGainBound, loopGain(nodes, stack.data() + first, stack.size() - first));
    if (!any) unbreakable = true;
  }

  bool visit(int id) {   // false: `id` is being processed (the edge that led here is a feedback edge)
    if (color[id] == 2) return true;
    if (color[id] == 1) {
      closeLoop(id);
      return false;
    }
    color[id] = 1;
    entry.push_back({id, stack.empty() ? -1 : stack.back()});
    stack.push_back(id);
    NodeS& nd = *nodes[id];
    nd.reachable = true;
    int lvl = 0, dep = 0;
    forEachUpstream(nd, [&](int up) {
      if (!visit(up)) return;
      const NodeS& u = *nodes[up];
      lvl = std::max(lvl, u.level + 1);
      dep = std::max(dep, u.depth + (hasImpulseResponse(u) ? 1 : 0));
    });
    nd.level = lvl;
    nd.depth = dep;
    color[id] = 2;
    stack.pop_back();
    order.push_back(id);
    return true;
  }
};

// The second walk (option "cycle_delay_split"): edges OUT of a cut DelayNode carry no ordering -- is anything still cyclic?
struct CutWalk {
  const NodeTable& nodes;
  const std::vector<char>& candidate;
  std::vector<int> color, order, deferred, level, depth;
  bool cyclic = false;

  void visit(int id) {
    if (color[id] == 2 || cyclic) return;
    if (color[id] == 1) {
      cyclic = true;
      return;
    }
    color[id] = 1;
    int lvl = 0, dep = 0;
    forEachUpstream(*nodes[id], [&](int up) {
      if (candidate[up]) {   // the reader: a source (planned in front of everything); its writer is walked as a root of its own
        if (color[up] == 0) deferred.push_back(up);
        return;
      }
      visit(up);
      lvl = std::max(lvl, level[up] + 1);
      dep = std::max(dep, depth[up] + (hasImpulseResponse(*nodes[up]) ? 1 : 0));
    });
    level[id] = lvl;
    depth[id] = dep;
    color[id] = 2;
    order.push_back(id);
  }
};

// ---- loops that can be cut at a DelayNode (option "cycle_delay_split") ----
// A DelayNode whose delay is a constant of d >= 128 K samples reads, for any K consecutive blocks, only samples its ring held
// BEFORE those blocks: its output for the whole K-block chunk can be produced first (a gather from the history: the READER, a node
// without inputs), and its input appended afterwards (the WRITER).  With every loop cut that way the chunk's graph is acyclic; the
// reference's stale edge becomes an ordinary edge that reads its producer ONE BLOCK LATE (Exec::resolveInSeg).  Chunks of K blocks
// instead of one: a 0.25 s echo renders 93 blocks per chunk.
void cutLoops(NodeTable& nodes, const TopologyOptions& o, const std::vector<char>& candidate, Topology& t, std::vector<int>& order) {
  int K = 1 << 30;
  for (size_t m = 0; m < candidate.size(); m++)
    if (candidate[m]) K = std::min(K, splittable(*nodes[m], o.sampleRate));
  CutWalk w{nodes, candidate, std::vector<int>(nodes.size(), 0), {}, {}, std::vector<int>(nodes.size(), 0), std::vector<int>(nodes.size(), 0)};
  w.visit(0);
  for (size_t q = 0; q < w.deferred.size() && !w.cyclic; q++) w.visit(w.deferred[q]);
  if (w.cyclic || K < 2 || w.order.size() != order.size()) return;
  order = w.order;
  for (int id : order) {
    nodes[id]->level = w.level[id];
    nodes[id]->depth = w.depth[id];
    if (nodes[id]->type == GA_NODE_DELAY) rec<DelayS>(*nodes[id]).delaySplit = candidate[id] != 0;
  }
  t.cycleBlocks = K;
}

// The cone of a DelayNode: every node it reaches backwards.  One walk serves "is the delay on a loop" and the two acceptance passes.
struct ConeWalk {
  const NodeTable& nodes;
  std::vector<int> seen, work, cone;   // seen: the stamp of the last walk that reached the node
  const char* blocker = nullptr;       // why the last walk stopped: acceptanceBlocker's reason (nullptr: the cone reached the root again)
  int blockedAt = -1;

  // False when the walk stops: the cone reaches `root` again (rootFails), or holds what acceptanceBlocker names (blockers).  True: `cone`
  // is the whole cone, without the root.  skip: the edges (sorted, consumer << 32 | producer) the walk does not follow.
  bool run(int root, int stamp, const std::vector<uint64_t>* skip, bool rootFails, bool blockers) {
    if (seen.empty()) seen.assign(nodes.size(), -1);
    bool ok = true;
    cone.clear();
    work.assign(1, root);
    seen[root] = stamp;
    while (!work.empty() && ok) {
      const int from = work.back();
      work.pop_back();
      forEachUpstream(*nodes[from], [&](int up) {
        if (rootFails && up == root && ok) {
          ok = false;
          blocker = nullptr;
          blockedAt = up;
        }
        if (seen[up] == stamp || (skip && std::binary_search(skip->begin(), skip->end(), ((uint64_t)from << 32) | (uint64_t)up))) return;
        seen[up] = stamp;
        const char* why = blockers ? acceptanceBlocker(*nodes[up]) : nullptr;
        if (why && ok) {
          ok = false;
          blocker = why;
          blockedAt = up;
        }
        cone.push_back(up);
        work.push_back(up);
      });
    }
    return ok;
  }
};

}  // namespace

void Topology::clearProbes(NodeTable& nodes) {
  for (int id : probeDelays)   // (the previous chunk's choice, if a failure kept it from being cleared: runTwoStageChunk)
    if (id < (int)nodes.size() && nodes[id]) rec<DelayS>(*nodes[id]).delayProbe = false;
  probeDelays.clear();
}

// the sources whose playbackRate a signal modulates and the cone of their modulation inputs (cached per graph version)
void Topology::updateRateCone(const NodeTable& nodes, uint64_t graphVersion, const std::vector<int>& order) {
  if (rateModsVersion == graphVersion && rateCone.size() == nodes.size()) return;
  rateMods.clear();
  for (int id : order)
    if (rateModulated(*nodes[id])) rateMods.push_back({id, 0});
  rateCone.assign(nodes.size(), 0);
  std::vector<int> stack;
  auto reach = [&](int up) {
    if (rateCone[up]) return;
    rateCone[up] = 1;
    stack.push_back(up);
  };
  for (const auto& pm : rateMods)
    for (const auto& m : nodes[pm.first]->params[pm.second].modulation) reach(m.first);
  while (!stack.empty()) {
    const NodeS& nd = *nodes[stack.back()];
    stack.pop_back();
    forEachUpstream(nd, reach);
  }
  rateModsVersion = graphVersion;
}

// The rate decides how many samples each block consumes and where a one-shot source ends, and the planner needs that before it can plan
// the rest: the modulation inputs' cone is rendered first (Context::runTwoStageChunk).  What cannot be split so is refused.
void Topology::refuseRateCone(const NodeTable& nodes, const std::vector<int>& order) const {
  for (const auto& pm : rateMods)
    if (rateCone[pm.first])
      fail(GA_ERR_UNSUPPORTED, "a modulated playbackRate depends on a source whose own playbackRate is modulated, or on its own output "
                               "(nested modulated rates / feedback through the rate) -- not on the device path");
  for (int id : order)
    if (rateCone[id] && nodes[id]->type == GA_NODE_CONVOLVER)
      fail(GA_ERR_UNSUPPORTED, "a ConvolverNode in front of a modulated playbackRate is not on the device path");
}

// ---- DelayNodes on a loop whose output flag this chunk reads from their samples (option "delay_flag_exact" = 2) ----
// In a chunk of ONE block with no loop cut, the edges that read a producer's previous block (staleEdges) resolve to kept blocks of the
// previous chunk and the other edges form a DAG: everything a delay D depends on in this block lies in front of it in the walk, and
// every consumer of D either comes after it or reads the block before, whose flag was read a block ago.  Accepted, while nothing has
// moved: a reachable D with its flag down that is on a loop (among the stack nodes of a back edge, or reached by its own cone) and not
// in front of a modulated playbackRate, whose cone over the edges that are not stale holds nothing acceptanceBlocker names -- the
// conditions of the delays on no loop (acceptDelays), on the smaller cone.  While one is accepted the chunk is one block and no loop
// is cut; the flag is sticky, so chunks of `cycleBlocks` blocks return once it is up.
void Topology::acceptLoopDelays(const NodeTable& nodes, uint64_t graphVersion, const std::vector<int>& order) {
  std::sort(staleEdges.begin(), staleEdges.end());
  ConeWalk w{nodes};
  for (int id : order) {
    if (nodes[id]->type != GA_NODE_DELAY) continue;
    const DelayS& d = rec<DelayS>(*nodes[id]);
    if (d.delayAudible) continue;
    // on a loop?  (the whole cone, as the acceptance of the other delays walks it)
    if (!d.delayOnLoop && w.run(id, id, nullptr, true, false)) continue;
    // (a second stamp per delay: the cone over the edges that are not stale)
    if (!w.run(id, id + (int)nodes.size(), &staleEdges, false, true)) {
      kept(*this, id, w.blockedAt, "on a loop, ", w.blocker, " in its cone");
      continue;
    }
    updateRateCone(nodes, graphVersion, order);
    if (!rateMods.empty() && rateCone[id]) {
      kept(*this, id, id, "on a loop, in front of a modulated rate");
      continue;
    }
    if (loopProbeCone.empty()) loopProbeCone.assign(nodes.size(), 0);
    for (int up : w.cone) loopProbeCone[up] = 1;
    loopProbeDelays.push_back(id);
  }
}

// reachability, level, convolver depth on the graph as it stands after the queued commands
void Topology::analyse(NodeTable& nodes, const TopologyOptions& o, uint64_t graphVersion, std::vector<int>& out) {
  out.clear();
  staleLeavers.clear();
  for (auto& np : nodes) {
    np->prevReachable = np->reachable;
    np->reachable = false;
    np->isProcessing = false;
    np->level = 0;
    np->depth = 0;
    if (np->type == GA_NODE_DELAY) {
      DelayS& dl = rec<DelayS>(*np);
      dl.delaySplit = false;
      dl.delayOnLoop = false;
    }
  }
  cycleBlocks = 1;
  loopGainBound = 0.0;
  staleEdges.clear();
  loopProbeDelays.clear();
  loopProbeCone.clear();
  for (int id : staleProducers)
    if (id < (int)nodes.size() && nodes[id]) nodes[id]->staleProducer = false;
  staleProducers.clear();
  DestinationWalk w{nodes, *this, o, out, std::vector<int>(nodes.size(), 0)};
  w.visit(0);
  refOrder = staleProducers.empty() ? std::vector<int>() : out;   // (the reference's processing order: Context::refOrderSensitivity)
  if (staleProducers.empty()) refEntry.clear();
  else refEntry.swap(w.entry);   // (where the walk enters a modulator cone: runTwoStageChunk)
  if (o.delayFlagExact >= 2 && !staleProducers.empty()) acceptLoopDelays(nodes, graphVersion, out);
  if (!staleProducers.empty() && !w.unbreakable && o.cycleDelaySplit && loopProbeDelays.empty()) cutLoops(nodes, o, w.candidate, *this, out);
  order = out;
  version = graphVersion;
  hasCycles = !staleProducers.empty();
  for (auto& np : nodes)
    if (np->prevReachable && !np->reachable && !np->disposed) staleLeavers.push_back(np->id);
}

void Topology::refreshSummary(const NodeTable& nodes, uint64_t graphVersion, const std::vector<int>& order) {
  if (statsVersion == graphVersion && statsSize == order.size()) return;
  maxDepth = maxLevel = 0;
  hasTimeNodes = hasConvolvers = hasOscillators = hasStreams = hasSpatial = false;
  for (int id : order) {
    const NodeS& nd = *nodes[id];
    maxDepth = std::max(maxDepth, nd.depth);
    maxLevel = std::max(maxLevel, nd.level);
    if (nd.type == GA_NODE_DELAY || nd.type == GA_NODE_STREAM_SOURCE) hasTimeNodes = true;
    if (nd.type == GA_NODE_STREAM_SOURCE) hasStreams = true;
    if (nd.type == GA_NODE_CONVOLVER) hasConvolvers = true;   // (with or without an impulse response: Buffer setters run in drain())
    if (nd.type == GA_NODE_OSCILLATOR) hasOscillators = true;
    if (nd.type == GA_NODE_SPATIAL_PANNER) hasSpatial = true;
  }
  statsVersion = graphVersion;
  statsSize = order.size();
}

// ---- DelayNodes whose output flag this chunk reads from their samples (option "delay_flag_exact"; runTwoStageChunk) ----
// The flag rises at the first output SAMPLE that is != 0f (DelayNode.cs:72,92,96-97), which the host cannot see: it predicts the flag
// from the flags of the blocks that went into the ring (Sim::process), never late, sometimes early.  A delay whose cone can be
// rendered ahead of the rest is rendered in stage 1 instead, and the block in which its samples raise the flag is read back
// (delay_onset_kernel).  Accepted, per chunk, while nothing has moved: a reachable DelayNode whose flag is down, that is on no
// feedback loop (not among the nodes of a back edge's loop, DelayS::delayOnLoop, and not reached by its own cone: deciding it would
// split the reference's walk inside a block), not in front of a modulated playbackRate, and with nothing acceptanceBlocker names in
// front of it.  Every other delay keeps the prediction (ga_stats.delay_flags_predicted).
bool Topology::acceptDelays(NodeTable& nodes, const TopologyOptions& o, const std::vector<int>& order, std::vector<char>& stage1) {
  if (!o.delayFlagExact || !hasTimeNodes) return false;
  ConeWalk w{nodes};
  auto accept = [&](int id, DelayS& d) {
    if (stage1.empty()) stage1.assign(nodes.size(), 0);
    stage1[id] = 1;
    d.delayProbe = true;
    d.delayShadow = false;
    d.delaySpans.clear();
    probeDelays.push_back(id);
  };
  for (int id : order) {
    if (nodes[id]->type != GA_NODE_DELAY) continue;
    DelayS& d = rec<DelayS>(*nodes[id]);
    if (std::find(loopProbeDelays.begin(), loopProbeDelays.end(), id) != loopProbeDelays.end()) {   // (a delay on a loop, accepted by acceptLoopDelays)
      accept(id, d);
      continue;
    }
    if (d.delayAudible) continue;
    if (d.delayOnLoop || d.delaySplit) {
      kept(*this, id, id, "on a loop");
      continue;
    }
    if (!rateMods.empty() && rateCone[id]) {
      kept(*this, id, id, "in front of a modulated rate");
      continue;
    }
    // (the cone reaches D itself: D is on a loop that the walk from the destination closed through a node it had finished already, so
    // D was never on the stack of a back edge -- a consumer of D would be stage 1's and read a view D does not hand out)
    if (!w.run(id, id, nullptr, true, true)) {
      kept(*this, id, w.blockedAt, w.blocker ? w.blocker : "on a loop closed through a finished node", w.blocker ? " in front of it" : "");
      continue;
    }
    accept(id, d);
    for (int up : w.cone) stage1[up] = 1;
  }
  if (loopProbeDelays.empty()) return false;
  for (size_t id = 0; id < loopProbeCone.size(); id++)
    if (loopProbeCone[id]) stage1[id] = 1;
  return true;
}

// A feedback loop lies entirely inside stage 1's set or entirely outside it (the set is closed upstream; a loop through a modulated
// source is refused, a delay on a loop is not accepted): a loop outside is stage 2's alone, the same walk from the destination as a
// one-pass chunk.  A loop inside is stage 1's, and stage 1 has to enter the set where the reference's walk does (Sim::evalProbe): the
// nodes of the set first reached from a node outside it, in the order the walk reaches them.
// (A chunk with an accepted delay on a loop, ChunkRun::loopProbe, has loops that lie partly in each stage: stage 1 walks from the
// destination and passes through the nodes outside the set, Sim::passThrough.  The driver asks for no roots then.)
std::vector<int> Topology::coneRoots(const std::vector<char>& stage1) const {
  std::vector<int> roots;
  bool coneLoop = false;
  for (int id : staleProducers) coneLoop = coneLoop || stage1[id];
  if (coneLoop)
    for (const auto& e : refEntry)
      if (stage1[e.first] && (e.second < 0 || !stage1[e.second])) roots.push_back(e.first);
  return roots;
}

}  // namespace ga
