// ga_topology.hpp -- the graph analysis of a chunk (ga_topology.cpp): which nodes the destination reaches and in what order, their
// levels and convolver depths, the feedback loops and where they can be cut, the DelayNodes whose flag a chunk may read from their
// samples, the sources with a modulated playbackRate and the cone in front of them.  Everything here works on the node table and a
// few plain options: no device, no Context.  Context::chunkTopology (ga_chunk.cpp) is the driver; tests/topology_main.cpp runs the
// module on the host alone.
#pragma once
#include <cstdint>
#include <memory>
#include <utility>
#include <vector>

namespace ga {

struct NodeS;
using NodeTable = std::vector<std::unique_ptr<NodeS>>;

struct TopologyOptions {
  int sampleRate;
  int delayFlagExact;     // option "delay_flag_exact" (0, 1, 2)
  bool cycleDelaySplit;   // option "cycle_delay_split"
};

// What the analysis found, kept from chunk to chunk (Context::topology).  Per-node results live on the node records: reachable, level,
// depth, staleProducer, DelayS::delaySplit / delayOnLoop / delayProbe.
struct Topology {
  uint64_t version = 0;     // the graph version `order` belongs to (connections / disposals / IR changes bump Context::graphVersion)
  std::vector<int> order;   // reachable nodes in planning (post) order
  int maxDepth = 0, maxLevel = 0;
  bool hasTimeNodes = false, hasConvolvers = false, hasOscillators = false, hasStreams = false, hasSpatial = false;
  uint64_t statsVersion = ~0ull;   // (the summary above is cached with the order: a sweep over 28,672 node records is 0.5 ms)
  size_t statsSize = 0;
  bool hasCycles = false;   // some node is pulled while it is being processed: chunks of ONE block (the reference's own granularity)
  std::vector<int> staleProducers;
  std::vector<int> staleLeavers;   // nodes that were evaluated in the previous chunk and are not in this one (an edit took them out of
                                   // the graph): their output buffers keep the last block, which a later loop through them would read
  double loopGainBound = 0.0;   // the largest estimated gain of a feedback loop: differences that enter it grow by 1 / (1 - gain)
  std::vector<int> refOrder;   // the reference-order walk of a graph with feedback (the planning order may cut loops at DelayNodes)
  std::vector<std::pair<int, int>> refEntry;   // ... the same walk's (node, the node it was first reached from, -1 = none) in entry order
  int cycleBlocks = 1;          // blocks per chunk of a graph with feedback (1 unless every loop is cut at a DelayNode)
  // delay_flag_exact = 2, a graph with feedback (walked every chunk): the edges of the reference's walk that read their producer's
  // previous block, as (consumer << 32 | producer), sorted; the DelayNodes on a loop accepted for this chunk and the union of their
  // cones over the other edges
  std::vector<uint64_t> staleEdges;
  std::vector<int> loopProbeDelays;
  std::vector<char> loopProbeCone;
  // sources whose k-rate playbackRate is modulated by a signal: (node, param), cached with the graph version, and the cone of nodes
  // their modulation inputs depend on (rendered by the first stage of a two-stage chunk)
  std::vector<std::pair<int, int>> rateMods;
  std::vector<char> rateCone;
  uint64_t rateModsVersion = ~0ull;
  std::vector<int> probeDelays;   // the DelayNodes accepted for the current chunk (DelayS::delayProbe)
  int64_t chunkNo = 0;            // (experiment builds: the chunk number on the GA_DEBUG_DELAY_FLAG trace lines)

  // The order is kept while no connection, disposal or impulse response changed.  A graph with feedback is walked again every chunk:
  // whether its loops can be cut at their DelayNodes depends on the delay times, which are parameters, not graph structure.
  bool cached(uint64_t graphVersion) const { return version == graphVersion && !order.empty() && !hasCycles; }

  void clearProbes(NodeTable& nodes);   // the previous chunk's DelayS::delayProbe marks
  // the whole analysis of a graph whose order is not cached: `out` (and `order`) become the planning order
  void analyse(NodeTable& nodes, const TopologyOptions& o, uint64_t graphVersion, std::vector<int>& out);
  void refreshSummary(const NodeTable& nodes, uint64_t graphVersion, const std::vector<int>& order);
  void updateRateCone(const NodeTable& nodes, uint64_t graphVersion, const std::vector<int>& order);
  void refuseRateCone(const NodeTable& nodes, const std::vector<int>& order) const;   // throws GA_ERR_UNSUPPORTED
  // option "delay_flag_exact": marks the DelayNodes this chunk reads (probeDelays) and adds them and their cones to `stage1`;
  // true: one of them is on a loop (value 2)
  bool acceptDelays(NodeTable& nodes, const TopologyOptions& o, const std::vector<int>& order, std::vector<char>& stage1);
  std::vector<int> coneRoots(const std::vector<char>& stage1) const;

 private:
  void acceptLoopDelays(const NodeTable& nodes, uint64_t graphVersion, const std::vector<int>& order);
};

}  // namespace ga
