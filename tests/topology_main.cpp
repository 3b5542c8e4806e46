// Host-only check of the graph analysis (graphaudio_amd/csrc/ga_topology.cpp): small graphs are built from the library's own node
// records (ga::makeNode) at 48 kHz and analysed the way Context::chunkTopology drives the module; every expectation follows from the
// rules in the module's comments or from a value a GPU test pins (tests/test_gpu_cycles.py: 1, 4, 93 and 337 blocks per chunk).
// Prints the first difference and exits non-zero; `ok` on the last line otherwise.  No HIP call is made and no GPU is needed.
// tests/test_topology_host.py builds it with ga_topology.cpp under the address and undefined-behaviour sanitizers and runs it.
#include <cstdio>
#include <cstdlib>
#include <new>

#include "ga_engine.hpp"

using namespace ga;

#define CHECK(cond)                                                                   \
  do {                                                                                \
    if (!(cond)) {                                                                    \
      std::printf("%s:%d: %s: expected %s\n", __FILE__, __LINE__, gCase, #cond);       \
      std::exit(1);                                                                   \
    }                                                                                 \
  } while (0)

static const char* gCase = "";
static const int SR = 48000;
using Ids = std::vector<int>;

struct Graph {
  NodeTable nodes;
  Graph() { add(GA_NODE_DESTINATION); }
  int add(int type, double arg = 2.0) {
    nodes.push_back(makeNode(type, (int)nodes.size(), type == GA_NODE_DELAY ? 1.0 : arg, SR));
    return (int)nodes.size() - 1;
  }
  int gain(float g) {
    const int id = add(GA_NODE_GAIN);
    nodes[id]->params[0].value = g;
    return id;
  }
  int delay(float seconds) {
    const int id = add(GA_NODE_DELAY);
    nodes[id]->params[0].value = seconds;
    return id;
  }
  void connect(int src, int dst, int input = 0) { nodes[dst]->inputs[input].connected.push_back(Conn{src, 0}); }
  void modulate(int src, int dst, int param = 0) { nodes[dst]->params[param].modulation.push_back({src, 0}); }
  NodeS& operator[](int id) { return *nodes[id]; }
  DelayS& dl(int id) { return rec<DelayS>(*nodes[id]); }
};

// one chunk's analysis, in the order of Context::chunkTopology
struct Chunk {
  Ids order, roots;
  std::vector<char> stage1;
  bool loopProbe = false;
  Ids set() const {   // stage 1's nodes
    Ids s;
    for (size_t i = 0; i < stage1.size(); i++)
      if (stage1[i]) s.push_back((int)i);
    return s;
  }
};

static Chunk analyse(Graph& g, Topology& t, int flagExact = 0, bool split = true, uint64_t version = 1) {
  const TopologyOptions o{SR, flagExact, split};
  Chunk c;
  t.clearProbes(g.nodes);
  if (t.cached(version)) c.order = t.order;
  else t.analyse(g.nodes, o, version, c.order);
  t.refreshSummary(g.nodes, version, c.order);
  t.updateRateCone(g.nodes, version, c.order);
  if (!t.rateMods.empty()) {
    t.refuseRateCone(g.nodes, c.order);
    c.stage1 = t.rateCone;
  }
  c.loopProbe = t.acceptDelays(g.nodes, o, c.order, c.stage1);
  if (!c.stage1.empty() && !c.loopProbe) c.roots = t.coneRoots(c.stage1);
  return c;
}

static Ids sorted(Ids v) {
  std::sort(v.begin(), v.end());
  return v;
}

// destination <- mix gain <- {source, feedback gain <- delay <- mix gain}; `through`: a node type put between the mix and the delay
struct Echo : Graph {
  int mix, src, fb, d, mid = -1;
  explicit Echo(float seconds, int through = -1) {
    mix = gain(1.0f);
    src = add(GA_NODE_CONSTANT_SOURCE);
    fb = gain(0.55f);
    d = delay(seconds);
    connect(mix, 0);
    connect(src, mix);
    connect(fb, mix);
    connect(d, fb);
    if (through >= 0) {
      mid = add(through);
      connect(mix, mid);
      connect(mid, d);
    } else {
      connect(mix, d);
    }
  }
};

static void chainAndOrder() {
  gCase = "1 chain";
  Graph g;
  const int gn = g.gain(0.5f), bq = g.add(GA_NODE_BIQUAD), cs = g.add(GA_NODE_CONSTANT_SOURCE);
  g.connect(gn, 0);
  g.connect(bq, gn);
  g.connect(cs, bq);
  Topology t;
  const Chunk c = analyse(g, t);
  CHECK((c.order == Ids{cs, bq, gn, 0}));
  CHECK(g[cs].level == 0 && g[bq].level == 1 && g[gn].level == 2 && g[0].level == 3);
  for (auto& n : g.nodes) CHECK(n->depth == 0 && n->reachable);
  CHECK(!t.hasCycles && t.cycleBlocks == 1 && t.refOrder.empty() && t.staleProducers.empty() && t.maxLevel == 3 && t.maxDepth == 0);

  gCase = "2 parameters before inputs";
  Graph h;
  const int s = h.add(GA_NODE_CONSTANT_SOURCE), osc = h.add(GA_NODE_OSCILLATOR), a = h.gain(1.0f);
  h.connect(s, a);
  h.modulate(osc, a);
  h.connect(a, 0);
  Topology u;
  CHECK((analyse(h, u).order == Ids{osc, s, a, 0}));
}

static void convolverDepth() {
  gCase = "3 convolver depth";
  // an IrSpectra that owns no device memory, in static storage and never destroyed (its destructor is the header's one call into HIP)
  alignas(IrSpectra) static unsigned char room[sizeof(IrSpectra)];
  std::shared_ptr<IrSpectra> ir(new (room) IrSpectra, [](IrSpectra*) {});
  Graph g;
  const int s = g.add(GA_NODE_CONSTANT_SOURCE), c1 = g.add(GA_NODE_CONVOLVER), c2 = g.add(GA_NODE_CONVOLVER);
  g.connect(s, c1);
  g.connect(c1, c2);
  g.connect(c2, 0);
  rec<ConvolverS>(g[c1]).ir = ir;
  rec<ConvolverS>(g[c2]).ir = ir;
  Topology t;
  analyse(g, t);
  CHECK(g[s].depth == 0 && g[c1].depth == 0 && g[c2].depth == 1 && g[0].depth == 2 && t.maxDepth == 2 && t.hasConvolvers);
  rec<ConvolverS>(g[c1]).ir = nullptr;   // (an impulse response change bumps the graph version)
  analyse(g, t, 0, true, 2);
  CHECK(g[s].depth == 0 && g[c1].depth == 0 && g[c2].depth == 0 && g[0].depth == 1 && t.maxDepth == 1);
}

static void twoGains() {
  gCase = "4 two gains feeding each other";
  Graph g;
  const int g1 = g.gain(0.5f), s = g.add(GA_NODE_CONSTANT_SOURCE), g2 = g.gain(0.5f);
  g.connect(g1, 0);
  g.connect(s, g1);
  g.connect(g2, g1);
  g.connect(g1, g2);
  Topology t;
  const Chunk c = analyse(g, t);
  CHECK((t.staleProducers == Ids{g1}) && g[g1].staleProducer && !g[g2].staleProducer);
  CHECK(t.hasCycles && t.cycleBlocks == 1 && t.loopGainBound == 0.25);
  CHECK((t.refEntry == std::vector<std::pair<int, int>>{{0, -1}, {g1, 0}, {s, g1}, {g2, g1}}));
  CHECK(t.refOrder == c.order && (c.order == Ids{s, g2, g1, 0}));
}

static void echo() {
  gCase = "5 echo";
  const float seconds[4] = {0.001f, 0.0123f, 0.25f, 0.9f};
  const int blocks[4] = {1, 4, 93, 337};   // tests/test_gpu_cycles.py::test_echo_renders_in_chunks_of_the_delay
  for (int i = 0; i < 4; i++) {
    Echo g(seconds[i]);
    Topology t;
    const Chunk c = analyse(g, t);
    CHECK(t.hasCycles && t.cycleBlocks == blocks[i]);
    CHECK(g.dl(g.d).delaySplit == (blocks[i] > 1) && g.dl(g.d).delayOnLoop);
    CHECK(sorted(c.order) == sorted(t.refOrder) && c.order.size() == 5);
    CHECK((t.refOrder == Ids{g.src, g.d, g.fb, g.mix, 0}));
    if (blocks[i] > 1) CHECK((c.order == Ids{g.src, g.fb, g.mix, 0, g.d}));   // the reader is a source; the writer follows the mix
    analyse(g, t, 0, false);   // option "cycle_delay_split" off (the same Topology: it owns the nodes' staleProducer marks)
    CHECK(t.hasCycles && t.cycleBlocks == 1 && !g.dl(g.d).delaySplit);
  }
  Echo g(0.25f);
  g[g.d].params[0].events.push_back(ParamEvent{0, 0.25f, 0.f, 0.f, 0.0, 0.0});
  Topology t;
  analyse(g, t);
  CHECK(t.cycleBlocks == 1 && !g.dl(g.d).delaySplit);

  gCase = "6 two loops";
  Echo h(0.25f);
  const int fb2 = h.gain(0.4f), d2 = h.delay(0.0123f);
  h.connect(fb2, h.mix);
  h.connect(d2, fb2);
  h.connect(h.mix, d2);
  Topology u;
  analyse(h, u);
  CHECK(u.cycleBlocks == 4 && h.dl(h.d).delaySplit && h.dl(d2).delaySplit);
  const int a = h.gain(0.5f), b = h.gain(0.5f);   // a third loop that holds no DelayNode
  h.connect(a, h.mix);
  h.connect(b, a);
  h.connect(a, b);
  analyse(h, u, 0, true, 2);
  CHECK(u.cycleBlocks == 1 && !h.dl(h.d).delaySplit && !h.dl(d2).delaySplit);

  gCase = "7 feedback is walked every time";
  Echo k(0.25f);
  Topology v;
  analyse(k, v);
  CHECK(v.cycleBlocks == 93 && !v.cached(1));
  k[k.d].params[0].value = 0.0123f;   // a parameter, not graph structure: the version stays
  analyse(k, v);
  CHECK(v.cycleBlocks == 4);
  Graph plain;
  plain.connect(plain.add(GA_NODE_CONSTANT_SOURCE), 0);
  Topology w;
  CHECK(!w.cached(1));
  analyse(plain, w);
  CHECK(w.cached(1) && !w.cached(2));
  plain[1].reachable = false;   // (a cached graph is not walked: the mark stays as this line leaves it)
  CHECK((analyse(plain, w).order == Ids{1, 0}) && !plain[1].reachable);
}

static void flagExactOne() {
  gCase = "8 delay_flag_exact = 1, plain";
  {
    Graph g;
    const int s = g.add(GA_NODE_CONSTANT_SOURCE), d = g.delay(0.02f);
    g.connect(s, d);
    g.connect(d, 0);
    Topology t;
    Chunk c = analyse(g, t, 1);
    CHECK((t.probeDelays == Ids{d}) && g.dl(d).delayProbe && !c.loopProbe && (c.set() == Ids{s, d}) && c.roots.empty());
    CHECK(analyse(g, t, 0).stage1.empty() && t.probeDelays.empty() && !g.dl(d).delayProbe);   // the option off; the marks are cleared
    g.dl(d).delayAudible = true;
    c = analyse(g, t, 1);
    CHECK(t.probeDelays.empty() && c.stage1.empty() && !g.dl(d).delayProbe);
  }
  gCase = "8 two delays in a row";
  {
    Graph g;
    const int s = g.add(GA_NODE_CONSTANT_SOURCE), a = g.delay(0.02f), b = g.delay(0.01f);
    g.connect(s, a);
    g.connect(a, b);
    g.connect(b, 0);
    Topology t;
    const Chunk c = analyse(g, t, 1);
    CHECK((t.probeDelays == Ids{a}) && !g.dl(b).delayProbe && (c.set() == Ids{s, a}));
  }
  gCase = "8 a convolver in front";
  {
    Graph g;
    const int s = g.add(GA_NODE_CONSTANT_SOURCE), cv = g.add(GA_NODE_CONVOLVER), d = g.delay(0.02f);
    g.connect(s, cv);
    g.connect(cv, d);
    g.connect(d, 0);
    Topology t;
    CHECK(analyse(g, t, 1).stage1.empty() && t.probeDelays.empty());
  }
  gCase = "8 a modulated rate in front";
  {
    Graph g;
    const int s = g.add(GA_NODE_BUFFER_SOURCE), osc = g.add(GA_NODE_OSCILLATOR), d = g.delay(0.02f);
    g.modulate(osc, s);
    g.connect(s, d);
    g.connect(d, 0);
    Topology t;
    const Chunk c = analyse(g, t, 1);
    CHECK(t.probeDelays.empty() && (c.set() == Ids{osc}));
  }
  gCase = "8 inside a rate modulator's cone";
  {
    Graph g;
    const int s = g.add(GA_NODE_BUFFER_SOURCE), osc = g.add(GA_NODE_OSCILLATOR), d = g.delay(0.02f);
    g.connect(osc, d);
    g.modulate(d, s);
    g.connect(s, 0);
    Topology t;
    const Chunk c = analyse(g, t, 1);
    CHECK(t.probeDelays.empty() && (c.set() == Ids{osc, d}));
  }
  gCase = "8 the echo graph";
  {
    Echo g(0.25f);
    Topology t;
    CHECK(analyse(g, t, 1).stage1.empty() && t.probeDelays.empty() && t.cycleBlocks == 93);
  }
}

// tests/test_gpu_delay_flag_exact.py::delay_on_a_loop_closed_through_a_finished_node
struct Closed : Graph {
  int s, x, y, w;
  Closed() {
    s = add(GA_NODE_CONSTANT_SOURCE);
    x = gain(1.0f);
    y = gain(0.4f);
    w = delay(0.01f);
    connect(x, y);
    connect(y, x);
    connect(y, w);
    connect(w, x);
    connect(s, x);
    connect(x, 0);
  }
};

static void flagExactTwo() {
  gCase = "9 delay_flag_exact = 2, echo";
  {
    Echo g(0.25f);
    Topology t;
    Chunk c = analyse(g, t, 2);
    CHECK((t.loopProbeDelays == Ids{g.d}) && (t.probeDelays == Ids{g.d}) && c.loopProbe && c.roots.empty());
    CHECK(t.cycleBlocks == 1 && !g.dl(g.d).delaySplit);
    CHECK((t.staleEdges == std::vector<uint64_t>{((uint64_t)g.d << 32) | (uint64_t)g.mix}));
    CHECK((c.set() == Ids{g.d}));   // the delay's one edge is the stale one: its cone over the others is empty
    g.dl(g.d).delayAudible = true;
    c = analyse(g, t, 2);
    CHECK(t.loopProbeDelays.empty() && t.probeDelays.empty() && !c.loopProbe && c.stage1.empty() && t.cycleBlocks == 93);
  }
  gCase = "9 a tap in the cone";
  {
    Echo g(0.25f, GA_NODE_GAIN);   // mix -> gain -> delay: the stale edge is gain -> mix, the delay's cone holds the gain
    const int s2 = g.add(GA_NODE_CONSTANT_SOURCE);
    g.connect(s2, g.d);
    Topology t;
    const Chunk c = analyse(g, t, 2);
    CHECK(c.loopProbe && (c.set() == sorted(Ids{g.d, g.mid, s2})) && t.cycleBlocks == 1);
  }
  gCase = "9 a convolver on the loop";
  {
    Echo g(0.25f, GA_NODE_CONVOLVER);
    Topology t;
    const Chunk c = analyse(g, t, 2);
    CHECK(t.loopProbeDelays.empty() && t.probeDelays.empty() && !c.loopProbe && t.cycleBlocks == 93);
  }
  gCase = "9 closed through a finished node";
  {
    Closed g;
    Topology t;
    Chunk c = analyse(g, t, 1);
    CHECK(!g.dl(g.w).delayOnLoop && t.probeDelays.empty() && c.stage1.empty());
    c = analyse(g, t, 2);
    CHECK((t.probeDelays == Ids{g.w}) && c.loopProbe && (c.set() == sorted(Ids{g.y, g.w})) && t.cycleBlocks == 1);
  }
}

static int refused(Graph& g) {
  Topology t;
  try {
    analyse(g, t);
  } catch (const Err& e) {
    return e.code;
  }
  return 0;
}

static void rateModulation() {
  gCase = "10 rate modulation";
  {
    Graph g;
    const int s = g.add(GA_NODE_BUFFER_SOURCE), a = g.gain(0.05f), osc = g.add(GA_NODE_OSCILLATOR);
    g.connect(osc, a);
    g.modulate(a, s);
    g.connect(s, 0);
    Topology t;
    const Chunk c = analyse(g, t);
    CHECK((t.rateMods == std::vector<std::pair<int, int>>{{s, 0}}) && (c.set() == Ids{a, osc}) && c.roots.empty());
  }
  gCase = "10 loop inside the cone";
  {
    Graph g;
    const int s = g.add(GA_NODE_BUFFER_SOURCE), g1 = g.gain(0.5f), osc = g.add(GA_NODE_OSCILLATOR), g2 = g.gain(0.5f);
    g.modulate(g1, s);
    g.connect(osc, g1);
    g.connect(g2, g1);
    g.connect(g1, g2);
    g.connect(s, 0);
    Topology t;
    const Chunk c = analyse(g, t);
    CHECK((c.set() == Ids{g1, osc, g2}) && (c.roots == Ids{g1}) && (t.staleProducers == Ids{g1}));
  }
  gCase = "10 refusals";
  {
    Graph g;   // a modulated rate that depends on a source whose own rate is modulated
    const int s = g.add(GA_NODE_BUFFER_SOURCE), m = g.add(GA_NODE_BUFFER_SOURCE), osc = g.add(GA_NODE_OSCILLATOR);
    g.modulate(osc, m);
    g.modulate(m, s);
    g.connect(s, 0);
    CHECK(refused(g) == GA_ERR_UNSUPPORTED);
    Graph h;   // a ConvolverNode in front of a modulated rate
    const int s2 = h.add(GA_NODE_BUFFER_SOURCE), cv = h.add(GA_NODE_CONVOLVER), o2 = h.add(GA_NODE_OSCILLATOR);
    h.connect(o2, cv);
    h.modulate(cv, s2);
    h.connect(s2, 0);
    CHECK(refused(h) == GA_ERR_UNSUPPORTED);
    Graph k;   // (and neither: nothing is refused)
    const int s3 = k.add(GA_NODE_BUFFER_SOURCE);
    k.modulate(k.add(GA_NODE_OSCILLATOR), s3);
    k.connect(s3, 0);
    CHECK(refused(k) == 0);
  }
}

int main() {
  chainAndOrder();
  convolverDepth();
  twoGains();
  echo();
  flagExactOne();
  flagExactTwo();
  rateModulation();
  std::printf("ok\n");
  return 0;
}
