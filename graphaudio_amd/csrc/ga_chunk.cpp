// ga_chunk.cpp -- the passes of one render chunk (see ga_engine.hpp, ga_chunk_internal.hpp): topology, control-plane simulation,
// per-chunk resources, execution and commit.  Node planning: ga_plan_nodes.cpp; convolver stages: ga_plan_conv.cpp; source timelines: ga_sources.cpp.
#include "ga_chunk_internal.hpp"

namespace ga {

// ======================================================================================================
// slabs: chunk-frame indexed float arrays handed to node outputs / mixed inputs for the duration of a chunk
// ======================================================================================================
// slabs are allocated in blocks of about 1 GiB: how many slabs of `slabBytes` one block holds
size_t slabsPerBlock(size_t slabBytes) {
  return slabBytes ? std::max<size_t>(8, std::min<size_t>(1024, ((size_t)1 << 30) / slabBytes)) : 0;
}

float* getSlab(Context& c) {
  if (c.slabFree.empty()) {
    size_t slabBytes = (size_t)c.slabFrames * sizeof(float);
    size_t count = slabsPerBlock(slabBytes);
    char* blk = (char*)c.dalloc(slabBytes * count);
    c.slabBlocks.push_back(blk);
    for (size_t i = 0; i < count; i++) {
      float* p = (float*)(blk + i * slabBytes);
      c.slabAll.push_back(p);
      c.slabFree.push_back(p);
    }
  }
  float* p = c.slabFree.back();
  c.slabFree.pop_back();
  return p;
}

void resetSlabs(Context& c, int64_t frames) {
  int64_t need = roundup(frames, 256);
  if (need > c.slabFrames) {
    c.syncStream();
    size_t oldBytes = (size_t)c.slabFrames * sizeof(float);
    for (void* p : c.slabBlocks) c.dfree(p, oldBytes * slabsPerBlock(oldBytes));
    c.slabBlocks.clear();
    c.slabAll.clear();
    c.slabFrames = need;
    c.slabGen++;
  }
  c.slabFree = c.slabAll;
}

// ======================================================================================================
// runChunk
// ======================================================================================================
const bool gaTiming = getenv("GA_TIMING") != nullptr;   // measurements only: host phase times per chunk on stderr

double nowMs() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

// A chunk is planned in passes that advance persistent control state (queued disposals, lagged channel counts and silence
// flags, overlap / history double buffers) before the first launch, so a failure after the simulation has started leaves
// the context between two blocks.  Such a failure is STICKY: every later render on this context returns
// GA_ERR_INVALID_OPERATION until the context is recreated (include/graphaudio_hip.h, "Errors").  Failures of the argument
// and graph checks that run before any state moves (disposed context, cycle, unsupported node) leave the context usable.
void Context::runChunk(int64_t n, float* const* bus) {
  if (faulted) fail(GA_ERR_INVALID_OPERATION, "context is faulted by an earlier render error (" + faultMsg + "); create a new context");
  chunkPhase = 0;
  try {
    const double t0 = gaTiming ? nowMs() : 0.0;
    runChunkImpl(n, bus);
    if (gaTiming) fprintf(stderr, "[ga]   chunk total on the host (incl. destructors): %.3f ms\n", nowMs() - t0);
  } catch (const Err& e) {
    if (chunkPhase > 0) {
      faulted = true;
      faultMsg = e.msg;
    }
    throw;
  } catch (...) {
    if (chunkPhase > 0) {
      faulted = true;
      faultMsg = "unexpected exception";
    }
    throw;
  }
}

// pass 1: the graph analysis (ga_topology.cpp) and what it refuses, while nothing has moved: every failure here leaves the context usable
void Context::chunkTopology(ChunkRun& r) {
  const TopologyOptions o{sampleRate, delayFlagExact, cycleDelaySplit};
  topology.chunkNo = stats.chunks;
  topology.clearProbes(nodes);
  if (topology.cached(graphVersion)) r.topo = topology.order;
  else topology.analyse(nodes, o, graphVersion, r.topo);
  // Feedback: the loop closes through the block a producer put out LAST.  Unless every loop can be cut at a DelayNode (chunks of
  // `cycleBlocks` blocks) nothing can be batched along time -- the chunk is one block, the reference's own granularity (a 10 s
  // render = 3,750 chunks: launch bound, ~0.1 - 0.3 ms each)
  if (topology.hasCycles) r.n = std::min<int64_t>(r.n, topology.cycleBlocks);
  topology.refreshSummary(nodes, graphVersion, r.topo);
  r.maxDepth = topology.maxDepth;
  r.maxLevel = topology.maxLevel;
  // a playbackRate modulated by a signal (AudioBufferSourceNode / AudioStreamSourceNode): a two-stage chunk (runTwoStageChunk)
  topology.updateRateCone(nodes, graphVersion, r.topo);
  if (!topology.rateMods.empty()) {
    topology.refuseRateCone(nodes, r.topo);
    for (const auto& pm : topology.rateMods) {
      if (nodes[pm.first]->type != GA_NODE_BUFFER_SOURCE) continue;
      BufferSourceS& nd = rec<BufferSourceS>(*nodes[pm.first]);
      if (!nd.loop || nd.bufId < 0 || !buffers[nd.bufId]) continue;
      const SrcGeom g = sourceGeom(*this, nd, *buffers[nd.bufId]);
      if (g.loopEndFrame <= g.loopStartFrame)   // (the replay's guard would fire inside the device walk: refused while nothing has moved)
        fail(GA_ERR_UNSUPPORTED, "source loop of zero length with resampling never finishes a block in the reference");
    }
    r.rateMods = topology.rateMods;
    r.stage1 = topology.rateCone;
  }
  r.loopProbe = topology.acceptDelays(nodes, o, r.topo, r.stage1);
  r.probeDelays = topology.probeDelays;
  if (!r.stage1.empty() && !r.loopProbe) r.coneRoots = topology.coneRoots(r.stage1);
  refuseSpatialPanners(r);
  fetchDeviceState();
}

// SpatialPannerNode: what the device path does not render is refused here, while nothing has moved
void Context::refuseSpatialPanners(const ChunkRun& r) {
  if (!topology.hasSpatial) return;
  const double increment = (double)kBlock / sampleRate;
  bool builtin = false;   // some node has no set of its own
  for (int id : r.topo) {
    if (nodes[id]->type != GA_NODE_SPATIAL_PANNER) continue;
    SpatialPannerS& nd = rec<SpatialPannerS>(*nodes[id]);
    // (decided here, on the graph as the chunk finds it: a modulator that ends inside the chunk is disconnected by the simulation,
    // and the blocks before that still read it)
    nd.spSignals = spatialSignalDriven(nd);
    const std::string who = "SpatialPannerNode " + std::to_string(id) + ": ";
    for (int p = 0; p < GA_SPATIAL_PARAM_COUNT; p++) {
      if (nd.params[p].modulation.empty()) continue;
      if (!spatialParamSignals)
        fail(GA_ERR_UNSUPPORTED, who + "a signal is connected to parameter " + std::to_string(p) + " (signals on the node's parameters are not on the device path)");
      if (p == 13 && !spatialOcclusion)   // (its values exist on the device alone: the host cannot show that occlusion stays at 0)
        fail(GA_ERR_UNSUPPORTED, who + "a signal is connected to occlusion (Steam Audio's occlusion / three-band transmission filters are not known here, "
                                       "and a signal's values cannot be shown to stay at 0)");
    }
    const PlayBuf* hb = hrirSetOf(nd.irBuf);
    if (!hb && !spatialBuiltinHrir) fail(GA_ERR_UNSUPPORTED, who + "no HRIR set assigned (the device path has no built-in set)");
    if (hb && ((hb->channels & 1) || hb->channels % (2 * std::max(nd.hrirAzimuths, 1)) != 0 || hb->length < 1 || hb->length > kSpatialMaxTaps))
      fail(GA_ERR_UNSUPPORTED, who + "the HRIR set does not fit hrirAzimuths (channels must be a multiple of 2 * hrirAzimuths, 1 .. 512 frames)");
    builtin = builtin || !hb;
    const ParamS& oc = nd.params[13];
    bool occluded = oc.events.empty() ? oc.value > 0.0f : false;
    if (!oc.events.empty()) {
      double t = currentTime;   // the accumulated block clock (AudioContextBase.cs:78-79), as chunkSimulate builds it
      for (int64_t b = 0; b < r.n && !occluded; b++, t += increment) occluded = param_value_at(oc.events.data(), (int)oc.events.size(), oc.value, t) > 0.0f;
    }
    if (occluded && !spatialOcclusion)
      fail(GA_ERR_UNSUPPORTED, who + "occlusion > 0 (Steam Audio's occlusion / three-band transmission filters are not known here)");
  }
  // Nothing is refused: which set every node renders this chunk with.  A node without a set of its own is on the built-in one (option
  // "spatial_builtin_hrir"), with that set's azimuth count whatever its own hrirAzimuths.  A node that was on another set in its last
  // chunk -- its own, or the built-in one before the radius changed or the option was switched -- had its HRIR set changed (DESIGN.md
  // section 2e): the next processed block uses its own filters alone, the input history carries over.
  if (builtin) ensureSpatialHeadSet();
  for (int id : r.topo) {
    if (nodes[id]->type != GA_NODE_SPATIAL_PANNER) continue;
    SpatialPannerS& nd = rec<SpatialPannerS>(*nodes[id]);
    const PlayBuf* hb = hrirSetOf(nd.irBuf);
    nd.spSet = hb ? hb : &spHeadSet;
    nd.spAzimuths = hb ? nd.hrirAzimuths : kSpatialHeadAzimuths;
    const uint64_t epoch = hb ? 0 : spHeadEpoch;
    if (nd.spSetEpoch != epoch) nd.spPrev.valid = false;
    nd.spSetEpoch = epoch;
  }
}

// The built-in set for the context's rate and the current head radius, made on the context's stream in front of the chunk that needs
// it.  A copy made for another radius is retired: launches of the chunk in flight may still read it, it is freed when the stream is
// next known to be idle (Context::freeRetired), so the memory held does not grow with the number of radius changes.
void Context::ensureSpatialHeadSet() {
  if (spHeadSet.dev && spHeadSetRadius == spatialHeadRadius) return;
  const int T = spatial_head_taps((double)sampleRate, spatialHeadRadius);
  if (spHeadSet.devBase) {
    retired.push_back({spHeadSet.devBase, spHeadSet.devBytes});
    spHeadSet.dev = nullptr;
    spHeadSet.devBase = nullptr;
    spHeadEpoch++;
  }
  spHeadSet.channels = 2 * kSpatialHeadDirs;
  spHeadSet.length = T;
  spHeadSet.stride = (T + 63) / 64 * 64;
  spHeadSet.sampleRate = sampleRate;
  spHeadSet.dev = dallocSkewed((size_t)spHeadSet.channels * (size_t)spHeadSet.stride * sizeof(float), &spHeadSet.devBase, &spHeadSet.devBytes);
  launch_spatial_head(stream, spHeadSet.dev, spHeadSet.stride, T, (double)sampleRate, spatialHeadRadius);
  GA_HIP(hipGetLastError());
  stats.kernel_launches++;
  spHeadSetRadius = spatialHeadRadius;
}

// SpatialPannerS::spGainBound of the nodes on the built-in set (the loop-gain estimate of the graph analysis reads it): max(1, the
// largest sum |p| sum |g| over the set's channels).  Only when the graph, the radius or the option moved since the nodes last got it.
void Context::spatialHeadBounds() {
  if (!spatialBuiltinHrir || (spHeadBoundVersion == graphVersion && spHeadBoundEpoch == spHeadEpoch && spHeadBoundRadius == spatialHeadRadius)) return;
  if (spHeadBoundRadius != spatialHeadRadius) {
    double mx = 1.0;
    for (int ch = 0; ch < 2 * kSpatialHeadDirs; ch++) mx = std::max(mx, spatial_head_abs_sum_bound(spatial_head_ear((double)sampleRate, spatialHeadRadius, ch)));
    spHeadGainBound = (float)(mx * (1.0 + 1e-6));
    spHeadBoundRadius = spatialHeadRadius;
  }
  bool moved = false;
  for (auto& np : nodes) {
    if (!np || np->disposed || np->type != GA_NODE_SPATIAL_PANNER) continue;
    SpatialPannerS& nd = rec<SpatialPannerS>(*np);
    if (nd.irBuf >= 0 || nd.spGainBound == spHeadGainBound) continue;
    nd.spGainBound = spHeadGainBound;
    moved = true;
  }
  if (moved) graphVersion++;   // (the analysis is cached per graph version)
  spHeadBoundVersion = graphVersion;
  spHeadBoundEpoch = spHeadEpoch;
}

// automated runs that ended hand their state back to the host (the one step of the pass that touches the device): only nodes whose
// state went to the device are looked at (Context::deviceStateNodes; "this chunk ran the per-sample kernel" is a stamp,
// DynStamp::dynSeq, not a flag to reset)
void Context::fetchDeviceState() {
  for (size_t i = 0; i < deviceStateNodes.size();) {
    const int id = deviceStateNodes[i];
    NodeS* np = id < (int)nodes.size() ? nodes[id].get() : nullptr;
    const bool onDevice = np && !np->disposed &&
                          ((np->type == GA_NODE_STEREO_PANNER && rec<StereoPannerS>(*np).panOnDevice) ||
                           (np->type == GA_NODE_BIQUAD && rec<BiquadS>(*np).coefOnDevice) ||
                           (np->type == GA_NODE_SPATIAL_PANNER && rec<SpatialPannerS>(*np).spOnDevice));
    if (!onDevice) {
      deviceStateNodes[i] = deviceStateNodes.back();
      deviceStateNodes.pop_back();
      continue;
    }
    i++;
    if (!np->reachable) continue;
    // (while a signal is connected to the parameter the node stays on its per-sample kernel, which serves a silent modulation input
    // as a constant too -- Sim::process -- so the state stays where it is: no stall of the pipeline per modulated node and chunk)
    if (np->type == GA_NODE_STEREO_PANNER) {
      StereoPannerS& nd = rec<StereoPannerS>(*np);
      if (!nd.params[0].events.empty() || !nd.params[0].modulation.empty()) continue;
      PanState tmp;   // back to a constant pan: the gains the automated run left on the device are the node's state
      syncStream();   // the state the previous chunk left
      GA_HIP(hipMemcpy(&tmp, nd.panDev, sizeof(PanState), hipMemcpyDeviceToHost));
      nd.panLast = tmp.last_pan;
      nd.panGL = tmp.gain_l;
      nd.panGR = tmp.gain_r;
      nd.panOnDevice = false;
      apiEpoch++;   // (host-tracked state changed: the next first block is traversed)
    } else if (np->type == GA_NODE_SPATIAL_PANNER) {
      SpatialPannerS& nd = rec<SpatialPannerS>(*np);
      if (spatialSignalDriven(nd)) continue;
      // the last signal is gone: the descriptor of the previous processed block comes back once, the host path continues (and its
      // first block fades from the descriptor the device made).  `valid` never left the host.
      if (nd.spPrev.valid && nd.spCarry[nd.spCarryCur]) {
        SpatialCarry tmp;
        syncStream();
        GA_HIP(hipMemcpy(&tmp, nd.spCarry[nd.spCarryCur], sizeof(SpatialCarry), hipMemcpyDeviceToHost));
        for (int q = 0; q < 4; q++) {
          nd.spPrev.idx[q] = tmp.idx[q];
          nd.spPrev.w[q] = tmp.w[q];
        }
        nd.spPrev.g = tmp.g;
        nd.spPrev.beta = tmp.beta;
        if (nd.spEqOnDevice && nd.spDirect) {   // ... and the previous triple with the run flags of the band filters
          SpatialDirectState ds;
          GA_HIP(hipMemcpy(&ds, nd.spDirect, sizeof(SpatialDirectState), hipMemcpyDeviceToHost));
          nd.spEq = ds.prev;
          nd.spEqOpen = (ds.open[0] ? 1 : 0) | (ds.open[1] ? 2 : 0);
        }
      }
      nd.spEqOnDevice = false;
      nd.spOnDevice = false;
      apiEpoch++;
    } else {
      BiquadS& nd = rec<BiquadS>(*np);
      if (!nd.bqDyn) continue;
      bool automated = false;
      for (auto& p : nd.params) automated = automated || !p.events.empty() || !p.modulation.empty();
      if (!automated) {  // back to constant parameters: fetch the coefficients the automated run left on the device
        BiquadDynState tmp;
        syncStream();
        GA_HIP(hipMemcpy(&tmp, nd.bqDyn, 24, hipMemcpyDeviceToHost));
        nd.b0 = tmp.b0; nd.b1 = tmp.b1; nd.b2 = tmp.b2; nd.a1 = tmp.a1; nd.a2 = tmp.a2;
        nd.coefDirty = tmp.dirty != 0;
        nd.coefOnDevice = false;
        apiEpoch++;
      }
    }
  }
}

// pass 2: block clock, source timelines, control-plane simulation -> segments (from here on control state moves)
void Context::chunkSimulate(ChunkRun& r) {
  std::vector<int>& topo = r.topo;
  int64_t& n = r.n;
  std::vector<double>& bt = r.bt;
  std::vector<int>& srcIds = r.srcIds;
  std::vector<SrcPlanOut>& srcPlans = r.srcPlans;
  r.tmTopo = nowMs();
  // ---- block clock (accumulated, AudioContextBase.cs:78-79) ----
  bt.assign(n + 1, 0.0);
  bt[0] = currentTime;
  const double increment = (double)kBlock / sampleRate;
  for (int64_t i = 0; i < n; i++) bt[i + 1] = bt[i] + increment;

  // ---- plan sources ----
  std::vector<int64_t> breaks;
  for (int id : topo) {
    NodeS& nd = *nodes[id];
    const bool scheduled = nd.type == GA_NODE_CONSTANT_SOURCE || nd.type == GA_NODE_OSCILLATOR;
    if (nd.type != GA_NODE_BUFFER_SOURCE && !scheduled) continue;
    if (r.srcIndex.empty()) r.srcIndex.assign(nodes.size(), -1);
    r.srcIndex[id] = (int)srcIds.size();
    srcIds.push_back(id);
    const RateModIn* rm = (id < (int)r.rmOf.size() && r.rmOf[id] >= 0) ? &r.rmIn[r.rmOf[id]] : nullptr;
    srcPlans.push_back(scheduled ? planScheduled(*this, nd, n, bt) : planSource(*this, rec<BufferSourceS>(nd), n, bt, rm));
    for (const SrcSpan& sp : schedOf(nd).spans)
      if (sp.b0 > 0 && sp.b0 < n) breaks.push_back(sp.b0);
    if (srcPlans.back().partialBlock >= 0) {
      breaks.push_back(srcPlans.back().partialBlock);
      if (srcPlans.back().partialBlock + 1 < n) breaks.push_back(srcPlans.back().partialBlock + 1);
    }
  }
  for (int id : topo) {   // AudioStreamNodeBase: replay on indices; a change of channel count / silence is a segment break
    if (nodes[id]->type != GA_NODE_STREAM_SOURCE) continue;
    StreamSourceS& nd = rec<StreamSourceS>(*nodes[id]);
    // (a modulated rate: the values the first stage read back)
    nd.stRateMod = (id < (int)r.rmOf.size() && r.rmOf[id] >= 0) ? r.rmIn[r.rmOf[id]].rates : nullptr;
    if (!nd.stRateMod && !nd.params.empty() && !nd.params[0].modulation.empty()) fail(GA_ERR_DEVICE, "internal: modulated stream rate without its values");
    streamReplay(nd, n, bt, false);
    r.streamIds.push_back(id);
    for (int64_t b = 1; b < n; b++)
      if (nd.stInfo[b].outCh != nd.stInfo[b - 1].outCh || nd.stInfo[b].silent != nd.stInfo[b - 1].silent) breaks.push_back(b);
  }
  if (r.pre)   // the second stage breaks where the first stage's segments do: the rendered nodes' views change there
    for (int64_t b : r.pre->preB0)
      if (b > 0 && b < n) breaks.push_back(b);
  if (r.pre)   // ... and where the samples of a DelayNode raised its output flag (option "delay_flag_exact")
    for (int id : r.pre->probeDelays)
      for (const DelayS::DelaySpan& sp : rec<DelayS>(*nodes[id]).delaySpans)
        if (sp.onset > 0 && sp.onset < n) breaks.push_back(sp.onset);
  std::sort(breaks.begin(), breaks.end());
  breaks.erase(std::unique(breaks.begin(), breaks.end()), breaks.end());
  std::unordered_map<int64_t, std::vector<int>> goneAt;
  for (size_t i = 0; i < srcIds.size(); i++)
    if (srcPlans[i].gone && srcPlans[i].goneAt < n) goneAt[srcPlans[i].goneAt].push_back(srcIds[i]);
  // The first stage of a two-stage chunk ends where one of its sources is disposed: a disposal disconnects the node from consumers the
  // second stage has yet to evaluate for the blocks before it.  (At block 0 both stages see it.)
  if (r.stage == 1)
    for (const auto& kv : goneAt)
      if (kv.first > 0) n = std::min(n, kv.first);

  r.tmSrc = nowMs();
  chunkPhase = 1;   // from here on persistent control state moves: a failure is sticky (see runChunk)
  // ---- simulate ----
  Sim sim{*this, n};
  sim.pre = r.pre;
  if (r.stage == 1 && r.loopProbe) sim.passSet = &r.stage1;
  std::vector<int64_t> extraBreaks;
  sim.extraBreaks = &extraBreaks;
  sim.blockTimes = &bt;
  int minDestCh = 32;
  if (r.stage == 1) {   // rows of the cone's output state in a snapshot (Sim::restorePre)
    r.preRow.assign(nodes.size(), -1);
    int row = 0;
    for (int id : topo) {
      r.preRow[id] = row;
      row += (int)nodes[id]->outputs.size();
    }
    // (an accepted delay's cone may change its channel count inside the chunk: the counts before the chunk, for stage 2's first block)
    if (!r.probeDelays.empty())
      for (int id : topo)
        for (const OutputS& o : nodes[id]->outputs) r.preCh0.push_back(o.bufCh);
  }
  {
    int64_t b = 0;
    uint64_t prevHash = lastHash;
    const size_t kMaxSegs = 96;
    while (b < n) {
      if (r.segs.size() >= kMaxSegs && r.stage != 2) {  // too fragmented: stop the chunk here, the caller continues with a new one
        // (not in the second stage of a two-stage chunk: the first stage has rendered its blocks)
        n = b;
        break;
      }
      auto g = goneAt.find(b);
      if (g != goneAt.end())
        for (int id : g->second) doDispose(id);  // queued Dispose() runs in the next block's DrainCommands
      Segment sg;
      sg.b0 = b;
      if (!segNodePool.empty()) {   // (storage of an earlier chunk's segment: warm, and no page faults of a fresh allocation)
        sg.nodes = std::move(segNodePool.back());
        segNodePool.pop_back();
      }
      sg.nodes.reserve(topo.size());
      sim.cur = &sg;
      sim.brel = b;
      sim.blockNumber = currentBlock + b + 1;
      // the first block of a steady chunk: nothing can have moved since the previous chunk's last segment (see Context::lastSegNodes)
      // -- its records are taken over, the traversal is skipped
      bool replayed = false;
      if (b == 0 && r.stage == 0 && simReplay && lastSegStable && !lastSegNodes.empty() && lastSegEpoch == apiEpoch && lastSegGraphVersion == graphVersion &&
          !topology.hasStreams && lastSegNodes.size() == topo.size() && g == goneAt.end()) {
        bool same = true;
        for (const NodeSeg& ns : lastSegNodes) {   // every source still in the phase (and on the buffer) the records say
          if (ns.type == GA_NODE_DELAY) {
            // a DelayNode's control state is its output flag, which is sticky once raised (DelayNode.cs:96-97): a node that is audible
            // with a constant delay time behaves like any other node; until then its ring model has to be walked block by block
            const DelayS& dn = rec<DelayS>(*nodes[ns.id]);
            if (!ns.delayAudible || !dn.delayAudible || !dn.params[0].events.empty() || !dn.params[0].modulation.empty()) {
              same = false;
              break;
            }
            continue;
          }
          if (ns.type != GA_NODE_BUFFER_SOURCE && ns.type != GA_NODE_CONSTANT_SOURCE && ns.type != GA_NODE_OSCILLATOR) continue;
          NodeS& sn = *nodes[ns.id];
          const SrcSpan& sp = spanAt(schedOf(sn), 0);
          if (sp.phase != ns.srcPhase || (ns.type == GA_NODE_BUFFER_SOURCE && ns.srcBuf != rec<BufferSourceS>(sn).bufId)) {
            same = false;
            break;
          }
        }
        if (same) {
          if (!sg.nodes.empty() || sg.nodes.capacity()) segNodePool.push_back(std::move(sg.nodes));
          sg.nodes = std::move(lastSegNodes);
          lastSegNodes.clear();
          for (NodeSeg& ns : sg.nodes) {
            switch (ns.type) {
              case GA_NODE_BUFFER_SOURCE:
                if (ns.srcPhase == SRC_PLAY) {
                  const SrcSpan& sp = spanAt(rec<BufferSourceS>(*nodes[ns.id]), 0);
                  ns.srcPos = sp.pos + (0 - sp.b0) * kBlock;
                  ns.srcBlk = sp.blkIdx + (0 - sp.b0);
                }
                break;
              case GA_NODE_BIQUAD:   // (per-chunk flags the traversal would have set again: Sim::process)
                if (ns.bqDynamic && !ns.ins[0].silent) rec<BiquadS>(*nodes[ns.id]).dynSeq = chunkSeq;
                break;
              case GA_NODE_STEREO_PANNER:
                if (ns.panDyn) rec<StereoPannerS>(*nodes[ns.id]).dynSeq = chunkSeq;
                break;
              case GA_NODE_DESTINATION:
                destOutCh = ns.outCh;
                break;
              default: break;
            }
          }
          sg.hash = lastSegHash;
          replayed = true;
          stats.sim_replays++;
        }
      }
      if (!replayed) {
        if (r.pre && !r.pre->preCh0.empty()) {
          // A consumer sizes its input from its producers' channel counts BEFORE it pulls them (AudioNodeInput.cs:140-168): the counts of
          // the block before.  Stage 1 has left the cone with the counts of the chunk's last block: put back what block b - 1 left.
          const ChunkRun& p = *r.pre;
          const size_t s1 = b > 0 ? (size_t)(std::upper_bound(p.preB0.begin(), p.preB0.end(), b - 1) - p.preB0.begin()) - 1 : 0;
          for (int id : p.topo) {
            NodeS& cn = *nodes[id];
            for (size_t o = 0; o < cn.outputs.size(); o++)
              cn.outputs[o].bufCh = b > 0 ? p.preSnap[s1][(size_t)p.preRow[id] + o].bufCh : p.preCh0[(size_t)p.preRow[id] + o];
          }
        }
        inRender = true;
        try {
          if (r.stage == 1) sim.evalProbe(r.rateMods, r.coneRoots, r.probeDelays);
          else sim.evalNode(0);
        } catch (...) {
          inRender = false;
          topology.version = 0;   // nodes may be left marked as processing: rebuild (and reset) everything next time
          throw;
        }
        inRender = false;
        for (int64_t x : extraBreaks)   // e.g. the block in which delayed audio reaches a DelayNode's output
          if (x > b && x < n) {
            auto it = std::lower_bound(breaks.begin(), breaks.end(), x);
            if (it == breaks.end() || *it != x) breaks.insert(it, x);
          }
        extraBreaks.clear();
        sg.hash = sim.hashSeg(sg);
      }
      lastSegStable = sg.hash == prevHash;   // (of the segment that turns out to be the chunk's last: a fixpoint of the traversal)
      int64_t nb;
      if (sg.hash != prevHash) {
        nb = b + 1;
      } else {
        auto it = std::upper_bound(breaks.begin(), breaks.end(), b);
        nb = it == breaks.end() ? n : *it;
      }
      sg.b1 = std::min(nb, n);
      prevHash = sg.hash;
      if (r.stage == 1) {   // the cone's output state in this segment, for the second stage (Sim::restorePre)
        std::vector<ChunkRun::PreOut> snap;
        for (int id : topo)
          for (const OutputS& o : nodes[id]->outputs) snap.push_back(ChunkRun::PreOut{o.bufCh, o.silent, o.zero});
        r.preSnap.push_back(std::move(snap));
        r.preB0.push_back(sg.b0);
      } else {
        minDestCh = std::min(minDestCh, sg.nodes.back().outCh);
      }
      b = sg.b1;
      r.segs.push_back(std::move(sg));
    }
    lastHash = prevHash;
    if (n < (int64_t)bt.size() - 1) {
      bt.resize(n + 1);
      // the chunk was cut short: the stream tables (window at the END of the chunk, pieces) are rebuilt for the blocks that run
      for (int id : r.streamIds) streamReplay(rec<StreamSourceS>(*nodes[id]), n, bt, false);
    }
  }
  if (r.pre && !r.pre->preCh0.empty() && !r.pre->preSnap.empty())   // (the cone leaves the chunk with the counts of its last block)
    for (int id : r.pre->topo)
      for (size_t o = 0; o < nodes[id]->outputs.size(); o++) nodes[id]->outputs[o].bufCh = r.pre->preSnap.back()[(size_t)r.pre->preRow[id] + o].bufCh;
  if (r.stage != 1) chunkMinDestCh = minDestCh;
  r.tmSim = nowMs();

}

// pass 3: per-chunk device resources (delay lines, slabs, zero page, bus)
void Context::chunkResources(ChunkRun& r) {
  const int64_t frames = r.n * kBlock;
  // ---- DelayNode state: history [rings][maxDelay] (persistent) and the chunk's line [rings][maxDelay + frames] ----
  for (int id : r.topo) {
    if (nodes[id]->type != GA_NODE_DELAY) continue;
    DelayS& nd = rec<DelayS>(*nodes[id]);
    nd.delayLoaded = false;
    int rings = std::max(nd.delayRings, 2);
    for (const Segment& sg : r.segs)
      for (const NodeSeg& ns : sg.nodes)
        if (ns.id == id) rings = std::max(rings, ns.ins[0].bufCh);   // EnsureChannelCount (:102-113): new rings start empty
    nd.delayRings = rings;
    const size_t maxD = (size_t)nd.maxDelaySamples;
    if (nd.delayHistRings < rings) {
      float* nh = (float*)dalloc(maxD * rings * sizeof(float));
      GA_HIP(hipMemsetAsync(nh, 0, maxD * rings * sizeof(float), stream));
      if (nd.delayHist) {
        GA_HIP(hipMemcpyAsync(nh, nd.delayHist, maxD * nd.delayHistRings * sizeof(float), hipMemcpyDeviceToDevice, stream));
        syncStream();
        dfree(nd.delayHist, maxD * nd.delayHistRings * sizeof(float));
      }
      nd.delayHist = nh;
      nd.delayHistRings = rings;
    }
    const int64_t cap = roundup(frames, 4096);
    if (nd.delayCap < cap || nd.delayLineRings < rings) {
      if (nd.delayLine) {
        syncStream();
        dfree(nd.delayLine, (maxD + (size_t)nd.delayCap) * nd.delayLineRings * sizeof(float));
      }
      nd.delayCap = std::max(nd.delayCap, cap);
      nd.delayLineRings = rings;
      nd.delayLine = (float*)dalloc((maxD + (size_t)nd.delayCap) * rings * sizeof(float));
    }
    nd.delayW.assign(rings, 0);
    nd.delayR.assign(rings, 0);
  }

  // ---- device resources for this chunk ----
  if (r.stage != 2) resetSlabs(*this, frames);   // (the second stage reads the first stage's slabs: none is handed out again)
  if (zerosLen < frames) {
    if (zeros) {
      syncStream();
      dfree(zeros, (size_t)zerosLen * 4);
    }
    zerosLen = roundup(frames, 4096);
    zeros = (float*)dalloc((size_t)zerosLen * 4);
    GA_HIP(hipMemsetAsync(zeros, 0, (size_t)zerosLen * 4, stream));
  }
  if (busCapFrames < frames) {
    syncStream();
    for (float* p : busSlabs) dfree(p, (size_t)busCapFrames * 4);
    busSlabs.clear();
    busCapFrames = roundup(frames, 4096);
  }
  while ((int)busSlabs.size() < 32 && (int)busSlabs.size() < std::max(destOutCh, 2)) busSlabs.push_back((float*)dalloc((size_t)busCapFrames * 4));
  {
    int mx = 0;
    for (auto& sg : r.segs)
      if (r.stage != 1) mx = std::max(mx, sg.nodes.back().outCh);
    while ((int)busSlabs.size() < mx) busSlabs.push_back((float*)dalloc((size_t)busCapFrames * 4));
  }

}

// pass 9: upload the job tables, enqueue every recorded launch in order, profile events
void Context::chunkExecute(ChunkRun& r) {
  int64_t& n = r.n;
  Exec& ex = *r.ex;
  r.tmPlan = nowMs();
  if (!pendingHandOver.empty()) {   // no pre-mix launch in this chunk took the previous chunk's hand-over along: copies in front
    std::vector<HandOver> hv;
    hv.swap(pendingHandOver);
    hipStream_t st = stream;
    ex.plan.launches.insert(ex.plan.launches.begin(), Plan::L{[hv, st](uint8_t*) {
      for (const HandOver& h : hv) GA_HIP(hipMemcpyAsync(h.dst_host, h.src, sizeof(float) * (size_t)h.n, hipMemcpyDeviceToHost, st));
    }, LK_OTHER, 0.0, 0.0});
  }
  // ---- upload tables, run ----
  ex.trajOffFinal = ex.plan.putv(ex.traj);
  ex.spatialJobsOff = ex.plan.putv(ex.spatialJobs);
  size_t tbytes = ex.plan.host.size();
  const int slot = asyncMode ? (int)(chunkSeq & 1) : 0;   // async: the other buffer may still be waiting for its upload
  void*& thost = slot ? tablesHostB : tablesHost;
  size_t& thostBytes = slot ? tablesHostBBytes : tablesHostBytes;
  if (asyncMode && chunkDone[slot]) GA_HIP(hipEventSynchronize(chunkDone[slot]));   // chunk k - 2 is done: its staging is free
  if (thostBytes < tbytes) {
    if (thost) {
      syncStream();
      (void)hipHostFree(thost);
    }
    thostBytes = (tbytes + tbytes / 4 + 4096 + 15) & ~(size_t)15;
    GA_HIP(hipHostMalloc(&thost, thostBytes, hipHostMallocDefault));
  }
  // option "coarse_tail_stream" (ga_engine.hpp): upload + pre-mix on `stream`, the coarse stage behind them on stream2.  Every other
  // chunk waits for the tail its predecessor may have left there before it enqueues anything.
  const bool tailChunk = tailWanted && tailCandidate && ex.plan.launches.size() == 2 && ex.plan.launches[0].kind == GA_STAGE_COARSE_SECTION &&
                         ex.plan.launches[1].kind == LK_CINV;
  tailCandidate = false;
  if (tailChunk) ensureOverlapStream();
  else joinTail();
  // (the previous chunk's tail may still read the other arena; renders that never leave a tail keep to the one)
  DevArena& tdev = (tailWanted && slot) ? tablesB : tables;
  ensure(tdev, std::max(tablesHostBytes, tablesHostBBytes));
  std::memcpy(thost, ex.plan.host.data(), tbytes);
  if (tableUploadKernel) launch_table_upload(stream, tdev.p, thost, tbytes);   // (staging and arena sizes are multiples of 16)
  else GA_HIP(hipMemcpyAsync(tdev.p, thost, tbytes, hipMemcpyHostToDevice, stream));
  uint8_t* base = (uint8_t*)tdev.p;
  struct TailActive {   // (cleared on every way out)
    Context& c;
    ~TailActive() { c.tailActive = false; }
  } tailGuard{*this};
  tailActive = tailChunk;

  std::vector<std::pair<hipEvent_t, hipEvent_t>> evs;
  std::vector<int> evKind;
  std::vector<double> evBytes;
  hipEvent_t evBegin = nullptr, evEnd = nullptr;
  const bool profile = profileNow;   // (this chunk is one of the sampled ones: option "profile_every")
  if (profile) {
    GA_HIP(hipEventCreate(&evBegin));
    GA_HIP(hipEventCreate(&evEnd));
    GA_HIP(hipEventRecord(evBegin, stream));
  }
  for (auto& l : ex.plan.launches) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const hipStream_t ls = l.kind == LK_CINV ? tailStreamNow() : stream;   // (the stream the launch goes to)
    if (profile) {
      GA_HIP(hipEventCreate(&e0));
      GA_HIP(hipEventCreate(&e1));
      GA_HIP(hipEventRecord(e0, ls));
    }
    l.fn(base);
    if (profile) {
      GA_HIP(hipEventRecord(e1, ls));
      evs.push_back({e0, e1});
      evKind.push_back(l.kind);
      evBytes.push_back(l.bytes);
    }
    if (l.kind == GA_STAGE_COARSE_SECTION) continue;   // (a section counts its own launches, per kernel)
    stats.kernel_launches++;
    if (l.kind >= 0 && l.kind < 16) {
      stats.stage_launches[l.kind]++;
      stats.stage_bytes[l.kind] += l.bytes;
      stats.stage_flops[l.kind] += l.flops;
    }
  }
  for (auto& x : extraProf) {   // pieces timed inside a launch (formulation D's overlapped section)
    evs.push_back({x.e0, x.e1});
    evKind.push_back(x.kind);
    evBytes.push_back(x.bytes);
  }
  extraProf.clear();
  if (profile) GA_HIP(hipEventRecord(evEnd, tailStreamNow()));
  GA_HIP(hipGetLastError());
  r.tmLaunch = nowMs();
  if (profileNow) pendingProf.push_back(ProfBatch{evBegin, evEnd, std::move(evs), std::move(evKind), std::move(evBytes)});
  if (asyncMode) {
    if (!chunkDone[slot]) GA_HIP(hipEventCreateWithFlags(&chunkDone[slot], hipEventDisableTiming));
    GA_HIP(hipEventRecord(chunkDone[slot], tailStreamNow()));
    if (tailChunk) {
      GA_HIP(hipEventRecord(tailEv, stream2));
      tailPending = true;
    }
    harvestProfile(false);
  } else {
    syncStream();
    harvestProfile(true);
  }
  tailActive = false;
  chunkSeq++;
  if (gaTiming)
    fprintf(stderr, "[ga]   host detail: topo %.2f, sources %.2f, sim %.2f | resources %.2f, params %.2f, exec %.2f ms\n", r.tmTopo - r.tm0,
            r.tmSrc - r.tmTopo, r.tmSim - r.tmSrc, r.tmRes - r.tmSim, r.tmPre - r.tmRes, r.tmPlan - r.tmPre);
  if (gaTiming)
    fprintf(stderr, "[ga] chunk %lld blocks: sim %.2f ms, plan %.2f ms, enqueue %.2f ms, wait %.2f ms%s\n", (long long)n, r.tmSim - r.tm0,
            r.tmPlan - r.tmSim, r.tmLaunch - r.tmPlan, nowMs() - r.tmLaunch, tailChunk ? ", coarse stage on the second stream" : "");

}

// pass 10: commit the control state (source positions, Ended / Dispose bookkeeping, block clock) to the end of the chunk
void Context::chunkCommit(ChunkRun& r) {
  int64_t& n = r.n;
  std::vector<double>& bt = r.bt;
  std::vector<int>& srcIds = r.srcIds;
  // ---- commit the control state to the end of the chunk ----
  for (size_t i = 0; i < srcIds.size(); i++) {
    SrcPlanOut& po = r.srcPlans[i];
    if (nodes[srcIds[i]]->type != GA_NODE_BUFFER_SOURCE) {  // ConstantSourceNode / OscillatorNode: only the Ended + Dispose bookkeeping
      SchedState& s = schedOf(*nodes[srcIds[i]]);
      if (po.gone && po.goneAt <= n) {
        if (!s.endedRaised) endedQueue.push_back(srcIds[i]);
        s.endedRaised = true;
        if (po.goneAt == n) pending.push_back([this, id = srcIds[i]]() { doDispose(id); });
      }
      continue;
    }
    BufferSourceS& s = rec<BufferSourceS>(*nodes[srcIds[i]]);
    // recompute progress against the (possibly shortened) chunk
    if (s.spans.empty()) continue;
    int64_t firstPlay = -1;
    for (const SrcSpan& sp : s.spans)
      if ((sp.phase == SRC_PLAY || sp.phase == SRC_END) && firstPlay < 0) firstPlay = sp.b0;
    if (firstPlay < 0 || firstPlay >= n) continue;
    int64_t lastProcessed = n;
    if (po.gone && po.goneAt <= n) lastProcessed = po.goneAt;
    int64_t played = lastProcessed - firstPlay;
    PlayBuf* pb = s.bufId >= 0 ? buffers[s.bufId].get() : nullptr;
    bool rate1 = true;
    if (pb) rate1 = sourceGeom(*this, s, *pb).effectiveRate == 1.0;
    if (s.gsr && s.gsrWalked >= 0) {   // walked on the device (a modulated rate): the state after the walked blocks
      if (played == s.gsrWalked) {
        s.playbackPosition = s.gsrTail.pp;
        for (int k = 0; k < 4; k++) s.gsrW[k] = s.gsrTail.w[k];
        s.gsrPos = s.gsrTail.pos;
        s.gsrReady = s.gsrTail.ready;
      } else if (!(po.gone && po.goneAt <= n)) {   // (a source that is gone leaves nothing to resume)
        fail(GA_ERR_DEVICE, "internal: a walked source ends its chunk at another block than its walk");
      }
    } else if (s.gsr) {
      if (!s.gsrBlocks.empty()) {  // the state at the start of block `played` (END blocks leave nothing to resume)
        const GsrBlock& e = s.gsrBlocks[std::min<size_t>((size_t)played, s.gsrBlocks.size() - 1)];
        s.playbackPosition = e.pp;
        for (int k = 0; k < 4; k++) s.gsrW[k] = e.w[k];
        s.gsrPos = e.pos;
        s.gsrReady = e.ready;
      }
    } else if (rate1) {
      s.playbackPosition += played * kBlock;
      if (s.loop && pb) {
        SrcGeom g = sourceGeom(*this, s, *pb);
        int64_t len = g.loopEndFrame - g.loopStartFrame;
        if (s.playbackPosition >= g.loopEndFrame && len > 0)
          s.playbackPosition = g.loopStartFrame + ((s.playbackPosition - g.loopEndFrame) % len);
      }
    } else {
      s.rsBlocks += played;
    }
    if (po.reachedEnd && po.endBlock < n) {
      s.stopTime = bt[po.endBlock + 1];
      s.hasStopped = true;
    }
    if (po.gone && po.goneAt <= n) {
      if (!s.endedRaised) endedQueue.push_back(srcIds[i]);
      s.endedRaised = true;
      if (po.goneAt == n) pending.push_back([this, id = srcIds[i]]() { doDispose(id); });  // runs in the next block's drain
    }
  }
  for (int id : r.streamIds) streamReplay(rec<StreamSourceS>(*nodes[id]), n, bt, true);   // queue / resampler state at the end of the executed blocks
  if (r.stage == 1) return;   // (the second stage of the chunk advances the clock)
  currentBlock += n;
  currentTime = bt[n];
  stats.blocks_rendered = currentBlock;
  stats.chunks++;
  stats.segments += (int64_t)r.segs.size();
  chunkBlocksDone = n;
  chunkSegCh.clear();
  for (const Segment& sg : r.segs) chunkSegCh.push_back(SegCh{sg.b0, sg.b1, sg.nodes.back().outCh});
}

void Context::runChunkImpl(int64_t nblocks, float* const* /*unused*/) {
  ChunkRun r;
  r.n = nblocks;
  r.tm0 = nowMs();
  GA_HIP(hipSetDevice(device));
  if (disposed) fail(GA_ERR_DISPOSED, "context disposed");
  drain();  // AudioContextBase.cs:57
  if (!releasedPending.empty() || ++chunksSinceGc >= 64) collectGarbage();
  latched = true;
  profileNow = profile && (profileSeq++ % std::max(profileEvery, 1)) == 0;
  spatialHeadBounds();
  chunkTopology(r);
  if (!r.rateMods.empty() || !r.probeDelays.empty()) {   // a playbackRate modulated by a signal, a DelayNode's flag read from its samples: their cones first (runTwoStageChunk)
    runTwoStageChunk(r);
    return;
  }
  chunkSimulate(r);
  chunkResources(r);
  r.tmRes = nowMs();
  bqSplitUsed = 0;   // (the blocks are reused chunk after chunk: every use is ordered on the stream behind the previous one)
  r.ex = std::make_unique<Exec>(*this, r.n, r.segs);
  r.ex->outViews.resize(r.segs.size());
  r.ex->plan.host.resize(16);  // reserved header
  chunkStaleSeed(r);
  chunkParamCurves(r);
  const double tmPar = nowMs();
  chunkConvScratch(r);
  r.tmPre = nowMs();
  double tmNodes = 0, tmConv = 0;
  for (int d = 0; d <= r.maxDepth; d++) {   // stages: convolver depth d
    const double a = nowMs();
    chunkPlanNodes(r, d);
    const double b = nowMs();
    chunkPlanConvolvers(r, d);
    tmNodes += b - a;
    tmConv += nowMs() - b;
  }
  chunkDelayCommit(r);
  chunkStaleCommit(r);
  chunkExecute(r);
  const double tmEx = nowMs();
  chunkCommit(r);
  chunkRetire(r);
  if (gaTiming)
    fprintf(stderr, "[ga]   host detail: param curves %.3f, conv scratch %.3f, plan nodes %.3f, plan convolvers %.3f, commit %.3f ms\n",
            tmPar - r.tmRes, r.tmPre - tmPar, tmNodes, tmConv, nowMs() - tmEx);
}

// after the commit: the last segment's views and records stay for the next chunk, the other per-chunk tables go back to the pools
void Context::chunkRetire(ChunkRun& r) {
  // the last segment's output views stay for one chunk (Context::chunkStaleSeed); the other per-node tables go back to the pools
  if (!r.ex->outViews.empty() && !r.segs.empty()) {
    if (!lastViews.empty() && viewsPool.size() < 8) viewsPool.push_back(std::move(lastViews));
    lastViews = std::move(r.ex->outViews.back());
    r.ex->outViews.pop_back();
    const size_t sl = r.segs.size() - 1;
    if (sl < r.ex->outScale.size() && !r.ex->outScale[sl].empty()) lastViewScale = r.ex->outScale[sl];
    else lastViewScale.clear();
    if (sl < r.ex->outCurve.size() && !r.ex->outCurve[sl].empty()) lastViewCurve = r.ex->outCurve[sl];
    else lastViewCurve.clear();
    lastViewFrames = r.n * kBlock;
    lastViewSlabGen = slabGen;
  }
  for (auto& ov : r.ex->outViews)
    if (!ov.empty() && viewsPool.size() < 8) viewsPool.push_back(std::move(ov));
  if (!r.segs.empty() && simReplay) {   // the last segment's records stay: the next chunk may take them over (Context::lastSegNodes)
    if (lastSegNodes.capacity() && segNodePool.size() < 8) {
      lastSegNodes.clear();
      segNodePool.push_back(std::move(lastSegNodes));
    }
    lastSegNodes = std::move(r.segs.back().nodes);
    lastSegHash = r.segs.back().hash;
    lastSegEpoch = apiEpoch;
    lastSegGraphVersion = graphVersion;
    r.segs.pop_back();
  }
  for (Segment& sg : r.segs) {
    sg.nodes.clear();
    if (segNodePool.size() < 8) segNodePool.push_back(std::move(sg.nodes));
  }
  r.ex.reset();
}

// ======================================================================================================
// two-stage chunks: a k-rate playbackRate modulated by a signal, a DelayNode's output flag read from its samples
// ======================================================================================================
// The rate of every block (clamp(intrinsic(t0) + modulation[0]), AudioParam.cs:143-165) sets how many samples the block consumes and
// where a one-shot source runs out of data: source spans, segments and the silence flags downstream depend on audio the host never
// sees.  Stage 1 runs the ordinary passes over the modulator cone (chunkTopology: every node the modulation inputs depend on), mixes
// the modulation inputs, computes the rates (krate_probe_kernel) and walks the buffer sources on the device (gsr_walk_kernel); ONE
// wait, then the host reads the rates and the walk summaries back.  Stage 2 plans and runs everything else: the cone's nodes count as
// rendered -- their per-block state comes from stage 1's simulation (Sim::restorePre), their output views from stage 1's executor.
// Nothing of the next chunk overlaps this one's planning: the wait is on the whole of stage 1.
// Option "delay_flag_exact": the DelayNodes chunkTopology accepted and their cones are stage 1's as well.  Stage 1 keeps each one's
// predicted flag apart (DelayS::delayShadow) and plans the node as ever; where the prediction raises the flag inside the chunk,
// delay_onset_kernel looks for the first block of the node's output rows that holds a sample != 0f, and its word travels to the host
// with the rates.  Stage 2 sees the flag down before that block and up from it on (Sim::restorePre), breaks its segments there and
// hands the node's rows to its consumers from there on.  Without a modulated rate and without a predicted rise there is nothing to
// read back: the probe and the wait are skipped, the two stages are queued back to back.
// A graph with feedback: every loop lies inside the cone (stage 1's) or outside it (stage 2's), and both stages run the chunk's r.n
// blocks -- `cycleBlocks` when every loop is cut at a DelayNode, one otherwise (chunkTopology).  A stale term resolves in the stage that
// plans its consumer, which is its producer's stage.  The kept blocks of the stale producers and leavers of BOTH stages are seeded
// once, in front of stage 1 (nothing has overwritten the previous chunk's slabs yet), and committed once, behind stage 2: stage 2's
// output views hold the cone's views (and folded gains / gain curves) copied from stage 1, and its commit stamps NodeS::staleSeq with
// the chunk number the next chunk's seed checks -- a commit in stage 1 would carry the number before and be seeded over again.
// Option "delay_flag_exact" = 2, a delay on a loop accepted (ChunkRun::loopProbe, chunkTopology): the chunk is one block, no loop is
// cut, and the loop lies partly in each stage.  Stage 1 holds the delay and its cone over the edges that are not stale, and walks
// from the destination, passing through the other nodes (Sim::passThrough); a stale term across the split is the kept block seeded
// in front of stage 1.  The gather and the test of the delay's block are one launch (delay_probe_kernel, chunkRateProbe).
void Context::runTwoStageChunk(ChunkRun& r) {
  // ---- stage 1: the modulator cone ----
  ChunkRun r1;
  r1.stage = 1;
  r1.n = r.n;
  r1.tm0 = r.tm0;
  r1.maxDepth = r.maxDepth;
  r1.maxLevel = r.maxLevel;
  r1.rateMods = r.rateMods;
  r1.coneRoots = std::move(r.coneRoots);
  r1.probeDelays = r.probeDelays;
  r1.loopProbe = r.loopProbe;
  if (r.loopProbe) r1.stage1 = r.stage1;   // (Sim::passThrough)
  const std::vector<char>& stage1 = r.stage1;
  for (int id : r.topo)
    if (stage1[id]) r1.topo.push_back(id);
  lastSegStable = false;   // (no first-block replay on either side of the split: chunkSimulate)
  chunkSimulate(r1);
  chunkResources(r1);
  r1.tmRes = nowMs();
  bqSplitUsed = 0;
  r1.ex = std::make_unique<Exec>(*this, r1.n, r1.segs);
  r1.ex->outViews.resize(r1.segs.size());
  r1.ex->plan.host.resize(16);
  chunkStaleSeed(r1);   // (both stages' stale producers, and nodes an edit took out of the graph: before anything overwrites the slabs)
  curveListTopoSize = ~(size_t)0;   // (the curve list is cached per topology: the two stages have different ones)
  chunkParamCurves(r1);
  chunkConvScratch(r1);
  r1.tmPre = nowMs();
  for (int d = 0; d <= r1.maxDepth; d++) {
    chunkPlanNodes(r1, d);
    chunkPlanConvolvers(r1, d);
  }
  chunkDelayCommit(r1);
  chunkRateProbe(r1);
  chunkExecute(r1);
  if (r1.waited) {   // (no modulated rate, and no accepted delay whose flag can rise in this chunk: nothing to read back)
    const double tw0 = nowMs();
    syncStream();   // the rates, walk summaries and onset blocks (chunkRateProbe)
    if (gaTiming) fprintf(stderr, "[ga]   two-stage chunk: stage 1 wait %.3f ms\n", nowMs() - tw0);
  }
  // the accepted delays: the block in which each span's samples raised the flag; the flag the node leaves the chunk with is its last span's
  for (int id : r1.probeDelays) {
    DelayS& d = rec<DelayS>(*nodes[id]);
    bool read = false;
    for (DelayS::DelaySpan& sp : d.delaySpans) {
      if (sp.word < 0) continue;
      const int32_t v = r1.onsetWords[sp.word];
      if (v != std::numeric_limits<int32_t>::max()) sp.onset = v;
      read = true;
    }
    d.delayAudible = !d.delaySpans.empty() && d.delaySpans.back().onset != std::numeric_limits<int64_t>::max();
    if (read) stats.delay_flags_read++;
    // (a loop: a consumer that reads this node's previous block takes the flag from the node's output state, and stage 2 may hold no
    // consumer that puts it there -- Sim::restorePre)
    if (r.loopProbe && !d.outputs.empty()) d.outputs[0].silent = !d.delayAudible;
  }

  // ---- stage 2: everything else ----
  r.stage = 2;
  r.n = r1.n;
  r.pre = &r1;
  r.rmOf = std::move(r1.rmOf);
  r.rmIn = std::move(r1.rmIn);
  {
    std::vector<int> rest;
    rest.reserve(r.topo.size() - r1.topo.size());
    for (int id : r.topo)
      if (!stage1[id]) rest.push_back(id);
    r.topo.swap(rest);
  }
  chunkSimulate(r);
  chunkResources(r);
  r.tmRes = nowMs();
  bqSplitUsed = 0;   // (stage 1 has finished on the device)
  r.ex = std::make_unique<Exec>(*this, r.n, r.segs);
  Exec& ex = *r.ex;
  ex.outViews.resize(r.segs.size());
  ex.plan.host.resize(16);
  const Exec& ex1 = *r1.ex;
  for (size_t si = 0; si < r.segs.size(); si++) {   // the cone's output views (and folded gains / gain curves) of stage 1
    const size_t s1 = (size_t)(std::upper_bound(r1.preB0.begin(), r1.preB0.end(), r.segs[si].b0) - r1.preB0.begin()) - 1;
    ex.outViews[si].resize(nodes.size());
    for (int id : r1.topo) {
      if (s1 < ex1.outViews.size() && id < (int)ex1.outViews[s1].size()) ex.outViews[si][id] = ex1.outViews[s1][id];
      const float g = ex1.scaleOf((int)s1, id);
      if (g != 1.f) ex.setScale((int)si, id, g);
      if (const float* cv = ex1.curveOf((int)s1, id)) ex.setCurve((int)si, id, cv);
    }
    // an accepted delay: stage 1 wrote its rows for every segment (planDelay) and handed out no view; consumers see them from the
    // onset on (stage 2 breaks its segments there: chunkSimulate)
    for (int id : r1.probeDelays) {
      const DelayS::DelaySpan* sp = nullptr;
      for (const DelayS::DelaySpan& q : rec<DelayS>(*nodes[id]).delaySpans)
        if (q.b0 <= r.segs[si].b0) sp = &q;
      if (!sp) continue;
      Views v((size_t)std::max(sp->ch, 1), nullptr);
      if (r.segs[si].b0 >= sp->onset)
        for (int ch = 0; ch < sp->ch; ch++) v[ch] = r1.ex->nodeOut(id, ch);
      ex.outViews[si][id] = v;
    }
  }
  curveListTopoSize = ~(size_t)0;
  chunkParamCurves(r);
  chunkConvScratch(r);
  r.tmPre = nowMs();
  for (int d = 0; d <= r.maxDepth; d++) {
    chunkPlanNodes(r, d);
    chunkPlanConvolvers(r, d);
  }
  chunkDelayCommit(r);
  chunkStaleCommit(r);   // (both stages' stale producers: see above)
  chunkExecute(r);
  chunkCommit(r1);   // (the cone's sources; the clock moves with stage 2's commit)
  chunkCommit(r);
  curveListTopoSize = ~(size_t)0;
  r1.ex.reset();
  for (int id : topology.probeDelays) rec<DelayS>(*nodes[id]).delayProbe = false;
  topology.probeDelays.clear();
  chunkRetire(r);
  lastSegStable = false;   // (the last segment's records hold stage 2's nodes only: no first-block replay in the next chunk)
}

// stage 1: the modulation input of every modulated rate mixed (Exec::resolveInSeg: the mix every modulated parameter gets), the rate
// of every block (krate_probe_kernel), the walk of every modulated buffer source (gsr_walk_kernel, option rate_mod_walk), the onset
// blocks of the accepted DelayNodes (delay_onset_kernel, option delay_flag_exact), and one copy of the rates, walk summaries and onset
// words to page-locked memory
void Context::chunkRateProbe(ChunkRun& r) {
  Exec& ex = *r.ex;
  const int64_t n = r.n;
  const int nm = (int)r.rateMods.size();
  std::vector<const float*> rows((size_t)nm * n, nullptr);
  for (size_t si = 0; si < r.segs.size(); si++) {
    const Segment& sg = r.segs[si];
    for (int k = 0; k < nm && k < (int)sg.probe.size(); k++) {
      const InSeg& is = sg.probe[k];
      if (is.silent) continue;   // the intrinsic value alone (AudioParam.cs:143-165)
      Views v = ex.resolveInSeg((int)si, r.rateMods[k].first, -1 - r.rateMods[k].second, is, false, nullptr);
      const float* row = (!v.empty() && v[0]) ? v[0] : zeros;
      for (int64_t b = sg.b0; b < sg.b1; b++) rows[(size_t)k * n + b] = row;
    }
  }
  ex.flushLevel();
  // walks
  std::vector<GsrWalkJob> walks;
  std::vector<int> walkOf(nm, -1), walkMod;
  if (rateModWalk)
    for (int k = 0; k < nm; k++) {
      NodeS& s = *nodes[r.rateMods[k].first];
      GsrWalkJob j{};
      if (s.type != GA_NODE_BUFFER_SOURCE || !rateModWalkJob(*this, rec<BufferSourceS>(s), n, r.bt, j)) continue;
      walkOf[k] = (int)walks.size();
      walkMod.push_back(k);
      walks.push_back(j);
    }
  // device area: rates [nm][n], walk summaries, descriptors; the first two are read back
  const size_t ratesBytes = (size_t)roundup((int64_t)nm * n * (int64_t)sizeof(float), 16);
  // the accepted delays (option "delay_flag_exact"): one job per span between two re-rents in which the prediction raises the flag --
  // the samples cannot raise it earlier -- over the blocks from there to the span's end; its word travels with the rates
  // (a one-block chunk with an accepted delay on a loop, delay_flag_exact = 2: planDelay has kept the gather of every such span back --
  // Exec::delayProbeJobs -- and delay_probe_kernel gathers, tests and lowers the word in one launch)
  std::vector<DelayOnsetJob> onsets;
  std::vector<int> onsetWord;   // the word of each job
  size_t nwords = 0;
  for (int id : r.probeDelays) {
    DelayS& d = rec<DelayS>(*nodes[id]);
    for (size_t k = 0; k < d.delaySpans.size(); k++) {
      DelayS::DelaySpan& sp = d.delaySpans[k];
      const int64_t end = std::min<int64_t>(k + 1 < d.delaySpans.size() ? d.delaySpans[k + 1].b0 : n, n);
      sp.word = -1;
      if (sp.rise < 0 || sp.rise >= end || sp.ch < 1) continue;
      bool fused = false;
      for (size_t q = 0; q < ex.delayProbeNode.size(); q++)
        if (ex.delayProbeNode[q] == id) fused = true;
      if (fused) {
        sp.word = (int)nwords++;
        continue;
      }
      DelayOnsetJob oj{};
      oj.nrows = std::min(sp.ch, kDelayOnsetRows);
      for (int ch = 0; ch < oj.nrows; ch++) oj.rows[ch] = ex.nodeOut(id, ch);   // (planDelay wrote every block of the span)
      oj.first = (int32_t)sp.rise;
      oj.count = (int32_t)(end - sp.rise);
      sp.word = (int)nwords++;
      onsetWord.push_back(sp.word);
      onsets.push_back(oj);
    }
  }
  const size_t onsetOff = (size_t)roundup((int64_t)(ratesBytes + walks.size() * sizeof(GsrWalkOut)), 16);
  const size_t readBytes = nwords == 0 ? ratesBytes + walks.size() * sizeof(GsrWalkOut)
                                       : (size_t)roundup((int64_t)(onsetOff + nwords * sizeof(int32_t)), 16);
  r.waited = readBytes > 0;
  if (!r.waited) return;
  size_t descCount = 0;
  for (const GsrWalkJob& j : walks) descCount += (size_t)j.nrel + 1;
  const size_t devBytes = readBytes + descCount * sizeof(GsrBlock);
  if (rateModDevBytes < devBytes) {
    if (rateModDev) {
      syncStream();   // (the previous chunk's gsr_kernel may still read its descriptors)
      dfree(rateModDev, rateModDevBytes);
    }
    rateModDevBytes = devBytes + devBytes / 2 + 4096;
    rateModDev = dalloc(rateModDevBytes);
  }
  if (rateModHostBytes < readBytes) {
    if (rateModHost) (void)hipHostFree(rateModHost);   // (nothing reads it outside the chunk that wrote it)
    rateModHostBytes = readBytes + readBytes / 2 + 4096;
    GA_HIP(hipHostMalloc(&rateModHost, rateModHostBytes, hipHostMallocDefault));
  }
  float* ratesDev = (float*)rateModDev;
  GsrWalkOut* outsDev = (GsrWalkOut*)((char*)rateModDev + ratesBytes);
  GsrBlock* descDev = (GsrBlock*)((char*)rateModDev + readBytes);
  const float* ratesHost = (const float*)rateModHost;
  const GsrWalkOut* outsHost = (const GsrWalkOut*)((const char*)rateModHost + ratesBytes);
  size_t d0 = 0;
  for (size_t w = 0; w < walks.size(); w++) {
    GsrWalkJob& j = walks[w];
    j.rates = ratesDev + (size_t)walkMod[w] * n;
    j.desc = descDev + d0;
    j.out = outsDev + w;
    d0 += (size_t)j.nrel + 1;
  }
  // what stage 2 plans the modulated sources with
  r.rmOf.assign(nodes.size(), -1);
  r.rmIn.assign(nm, RateModIn{});
  for (int k = 0; k < nm; k++) {
    RateModIn& m = r.rmIn[k];
    m.rates = ratesHost + (size_t)k * n;
    if (walkOf[k] >= 0) {
      const GsrWalkJob& j = walks[walkOf[k]];
      m.walk = outsHost + walkOf[k];
      m.desc = j.desc;
      m.nrel = j.nrel;
    }
    r.rmOf[r.rateMods[k].first] = k;
  }
  // the probe
  std::vector<KrateProbeJob> pjobs(nm);
  const size_t rowsOff = ex.plan.putv(rows);
  for (int k = 0; k < nm; k++) {
    const ParamS& ps = nodes[r.rateMods[k].first]->params[r.rateMods[k].second];
    KrateProbeJob& pj = pjobs[k];
    pj.rows_off = rowsOff + (size_t)k * n * sizeof(const float*);
    pj.events_off = ex.plan.putv(ps.events);
    pj.nev = (int)ps.events.size();
    pj.value = ps.value;
    pj.vmin = ps.minv;
    pj.vmax = ps.maxv;
    pj.pad_ = 0;
    pj.out = ratesDev + (size_t)k * n;
  }
  const size_t btOff = ex.plan.putv(r.bt);
  hipStream_t st = stream;
  if (nwords > 0) {
    int32_t* wordsDev = (int32_t*)((char*)rateModDev + onsetOff);
    r.onsetWords = (const int32_t*)((const char*)rateModHost + onsetOff);
    for (size_t k = 0; k < onsets.size(); k++) onsets[k].out = wordsDev + onsetWord[k];
    for (size_t q = 0; q < ex.delayProbeJobs.size(); q++) {   // (all rows of a node lower the node's word)
      const DelayS& d = rec<DelayS>(*nodes[ex.delayProbeNode[q]]);
      if (d.delaySpans.empty() || d.delaySpans.back().word < 0) fail(GA_ERR_DEVICE, "internal: a delay probe job without a word");
      ex.delayProbeJobs[q].word = wordsDev + d.delaySpans.back().word;
    }
    ex.delayProbeNode.clear();
    const std::vector<int32_t> none(nwords, std::numeric_limits<int32_t>::max());
    const size_t noneOff = ex.plan.putv(none), noneBytes = none.size() * sizeof(int32_t);
    ex.plan.add(LK_OTHER, [=](uint8_t* base) { GA_HIP(hipMemcpyAsync(wordsDev, base + noneOff, noneBytes, hipMemcpyDeviceToDevice, st)); });
    ex.flush(onsets, LK_OTHER, &DelayOnsetJob::count, [=](const DelayOnsetJob* t, int nj, int64_t mx, uint8_t*) { launch_delay_onset(st, t, nj, mx); });
    ex.flush(ex.delayProbeJobs, LK_OTHER, nullptr, [=](const DelayProbeJob* t, int nj, int64_t, uint8_t*) { launch_delay_probe(st, t, nj); });
  }
  ex.flush(pjobs, LK_OTHER, nullptr, [=](const KrateProbeJob* t, int nj, int64_t, uint8_t* base) { launch_krate_probe(st, t, nj, base, (const double*)(base + btOff), n); });
  ex.flush(walks, LK_OTHER, nullptr, [=](const GsrWalkJob* t, int nw, int64_t, uint8_t*) { launch_gsr_walk(st, t, nw); });
  void* hostDst = rateModHost;
  const void* devSrc = rateModDev;
  ex.plan.add(LK_OTHER, [=](uint8_t*) { GA_HIP(hipMemcpyAsync(hostDst, devSrc, readBytes, hipMemcpyDeviceToHost, st)); });
}

}  // namespace ga
