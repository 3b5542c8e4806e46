// Host-only probe of the node records (graphaudio_amd/csrc/ga_engine.hpp): for every node type the record is made by the factory the
// library uses (ga::makeNode), under a counting operator new, and destroyed the way Context::nodes destroys it -- through a
// unique_ptr<NodeS>.  One line per type:
//   record <type> sizeof <bytes> allocs <n> bytes <total> first <bytes of the first allocation> vectors <non-empty vectors> live <allocations left after destruction>
// then `common <sizeof(NodeS)>`, and the typed accessor called with the wrong type (`mismatch <code> <message>`, or `returned`).
// No HIP call is made and no GPU is needed.  tests/test_node_records_host.py builds and reads it.
#include <cstdio>
#include <cstdlib>
#include <new>

static long gAllocs = 0, gBytes = 0, gFirst = 0, gLive = 0;

void* operator new(std::size_t n) {
  void* p = std::malloc(n ? n : 1);
  if (!p) throw std::bad_alloc();
  if (gAllocs++ == 0) gFirst = (long)n;
  gBytes += (long)n;
  gLive++;
  return p;
}
void operator delete(void* p) noexcept {
  if (p) gLive--;
  std::free(p);
}
void operator delete(void* p, std::size_t) noexcept {
  if (p) gLive--;
  std::free(p);
}

#include "ga_engine.hpp"

using namespace ga;

// sizeof of the record each type is expected to have.  This table is written by hand, not taken from the factory: what ties the two
// together is the test's `first == sizeof` (the factory's first allocation IS the record).  A type added to makeNode but not here
// is taken for the common record and fails there.
static size_t recordSize(int type) {
  switch (type) {
    case GA_NODE_BUFFER_SOURCE: return sizeof(BufferSourceS);
    case GA_NODE_CONSTANT_SOURCE: return sizeof(ConstantSourceS);
    case GA_NODE_OSCILLATOR: return sizeof(OscillatorS);
    case GA_NODE_STREAM_SOURCE: return sizeof(StreamSourceS);
    case GA_NODE_STEREO_PANNER: return sizeof(StereoPannerS);
    case GA_NODE_DELAY: return sizeof(DelayS);
    case GA_NODE_BIQUAD: return sizeof(BiquadS);
    case GA_NODE_CONVOLVER: return sizeof(ConvolverS);
    case GA_NODE_SPATIAL_PANNER: return sizeof(SpatialPannerS);
    default: return sizeof(NodeS);   // destination, gain, splitter, merger
  }
}

int main() {
  std::vector<std::unique_ptr<NodeS>> nodes;   // (as Context::nodes)
  nodes.reserve(1);
  for (int type = GA_NODE_DESTINATION; type <= GA_NODE_SPATIAL_PANNER; type++) {
    const double arg = type == GA_NODE_DELAY ? 1.0 : 2.0;   // (ga_node_create's defaults)
    gAllocs = gBytes = gFirst = gLive = 0;
    nodes.push_back(makeNode(type, 1, arg, 48000));
    const long allocs = gAllocs, bytes = gBytes, first = gFirst;
    const NodeS& n = *nodes.back();
    const int vectors = (n.inputs.empty() ? 0 : 1) + (n.outputs.empty() ? 0 : 1) + (n.params.capacity() ? 1 : 0);
    if (n.type != type || n.id != 1) return 2;
    nodes.clear();
    std::printf("record %d sizeof %zu allocs %ld bytes %ld first %ld vectors %d live %ld\n", type, recordSize(type), allocs, bytes, first, vectors, gLive);
  }
  std::printf("common %zu\n", sizeof(NodeS));
  std::unique_ptr<NodeS> gain = makeNode(GA_NODE_GAIN, 2, 2.0, 48000);
  try {
    DelayS& d = rec<DelayS>(*gain);
    std::printf("returned %d\n", d.maxDelaySamples);
  } catch (const Err& e) {
    std::printf("mismatch %d %s\n", e.code, e.msg.c_str());
  }
  try {
    std::printf("matched %d\n", rec<BiquadS>(*makeNode(GA_NODE_BIQUAD, 3, 2.0, 48000)).filterType);
    (void)schedOf(*gain);
    std::printf("returned\n");
  } catch (const Err& e) {
    std::printf("mismatch %d %s\n", e.code, e.msg.c_str());
  }
  return 0;
}
