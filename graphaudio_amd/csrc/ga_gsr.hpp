// ga_gsr.hpp -- general source replay (AudioBufferSourceNode.Process for ONE block on indices, see GsrBlock) as one set of
// __host__ __device__ statements: the host replays a source whose playbackRate follows a timeline (ga_sources.cpp, planSource),
// gsr_walk_kernel replays a source whose playbackRate is modulated by a signal (ga_kernels.hip).  Both builds use
// -ffp-contract=off: the host and the device run the same arithmetic and hand gsr_kernel the same descriptors.
#pragma once
#include "ga_kernels.hpp"

namespace ga {

// what a replay needs of the source and its buffer (sourceGeom, AudioBufferSourceNode.cs:165-185)
struct GsrGeom {
  int64_t loopStart, loopEnd, durEnd, len;
  double ratio;   // buffer sample rate / context sample rate
  int loop;
  int channels;   // of the buffer: a change (re)creates the resamplers (:238-245)
};

struct GsrState {
  int64_t w[4];     // buffer indices in S0..S3 (-1: never fed)
  double pos;       // CubicResampler.Pos
  int ready;        // CubicResampler.Ready
  int rsChannels;   // channel count the resamplers were made for
  int64_t pp;       // _playbackPosition
};

// status codes of a replay (GsrWalkOut::err)
enum : int {
  GSR_OK = 0,
  GSR_ERR_ZERO_LOOP = 1,   // a loop of zero length with resampling never finishes a block in the reference
  GSR_ERR_RESUMED = 2,     // a source resumed after an end block inside one render chunk
  GSR_ERR_WINDOW = 3,      // a window index outside the buffer
  GSR_ERR_FEED = 4,        // a fed index outside the buffer
};

__host__ __device__ inline void gsrFeed(GsrState& st, int64_t idx) {  // CubicResampler.Shift, :91-97
  st.w[0] = st.w[1];
  st.w[1] = st.w[2];
  st.w[2] = st.w[3];
  st.w[3] = idx;
}

// CubicResampler.Process (:26-63) on an index stream at(k), k < inLen
template <class At>
__host__ __device__ inline void gsrProcess(GsrState& st, At at, int inLen, int outLen, double rate, int& consumed, int& produced) {
  int inPos = 0, outPos = 0;
  while (st.ready < 4 && inPos < inLen) {
    gsrFeed(st, at(inPos++));
    st.ready++;
  }
  if (st.ready < 4) {
    consumed = inPos;
    produced = 0;
    return;
  }
  while (outPos < outLen) {
    int consume = (int)st.pos;
    if (inPos + consume > inLen) break;
    for (int i = 0; i < consume; i++) gsrFeed(st, at(inPos++));
    st.pos -= consume;
    outPos++;
    st.pos += rate;
  }
  consumed = inPos;
  produced = outPos;
}

// One block at the k-rate playbackRate `playbackRate`: fills the block's descriptor `d`, advances `st`.  `end` = the block is an END
// block (`!hasMoreData || (!_loop && _playbackPosition >= durationEndFrame)`, :360).  Returns a GSR_* status.
__host__ __device__ inline int gsrReplayBlock(const GsrGeom& g, float playbackRate, GsrState& st, GsrBlock& d, bool& end) {
  const double effectiveRate = g.ratio * playbackRate;
  const int64_t loopStart = g.loopStart, loopEnd = g.loopEnd, durEnd = g.durEnd, len = g.len;
  const bool loop = g.loop != 0;
  bool hasMore = false;
  int64_t first = -1;
  int outIdx = 0;
  d.pp = st.pp;
  d.rate = effectiveRate;
  d.pad_ = 0;
  auto snap = [&]() {
    for (int k = 0; k < 4; k++) d.w[k] = st.w[k];
    d.pos = st.pos;
    d.ready = st.ready;
  };
  if (effectiveRate == 1.0) {  // :186-235
    d.copy = 1;
    snap();
    int64_t pos = st.pp;
    while (outIdx < kBlock) {
      if (loop && pos >= loopEnd) pos = loopStart;
      if (pos >= durEnd && !loop) break;
      int64_t endFrame = loop ? loopEnd : (durEnd < len ? durEnd : len);
      int64_t av = endFrame - pos < (int64_t)(kBlock - outIdx) ? endFrame - pos : (int64_t)(kBlock - outIdx);
      int available = (int)av;
      if (available <= 0) break;
      if (first < 0) first = pos;
      pos += available;
      outIdx += available;
      hasMore = true;
    }
    st.pp += kBlock;
  } else {  // :236-358
    d.copy = 0;
    if (st.rsChannels != g.channels) {  // `_resamplers` (re)created and cleared (:238-245)
      st.w[0] = st.w[1] = st.w[2] = st.w[3] = -1;
      st.pos = 0.0;
      st.ready = 0;
      st.rsChannels = g.channels;
    }
    snap();
    int64_t pos = st.pp, consumedThis = 0;
    int guard = 0;
    while (outIdx < kBlock) {
      if (++guard > 4096) return GSR_ERR_ZERO_LOOP;
      if (loop && pos >= loopEnd) pos = loopStart;
      if (pos >= durEnd && !loop) break;
      int64_t endFrame = loop ? loopEnd : (durEnd < len ? durEnd : len);
      int available = (int)(endFrame - pos < len - pos ? endFrame - pos : len - pos);
      if (available <= 0) {
        if (loop) {
          pos = loopStart;
          consumedThis = pos - st.pp;
          continue;
        }
        break;
      }
      if (first < 0) first = pos;
      int consumed = 0, produced = 0;
      if (loop && pos + available >= loopEnd - 4) {  // the 512-sample wrap buffer (:297-314)
        const int64_t loopLength = loopEnd - loopStart;
        const int fromEnd = (int)(loopEnd - pos);
        const int needed = kBlock - outIdx + 4 < 512 ? kBlock - outIdx + 4 : 512;
        const int head = fromEnd < needed ? fromEnd : needed;
        const int64_t rest = needed - head > 0 ? needed - head : 0;
        const int tail = (int)(rest < loopLength ? rest : loopLength);
        const int64_t p0 = pos;
        gsrProcess(st, [=](int k) { return k < head ? p0 + k : loopStart + (k - head); }, head + tail, kBlock - outIdx, effectiveRate, consumed,
                   produced);
      } else {
        const int64_t p0 = pos;
        gsrProcess(st, [=](int k) { return p0 + k; }, available, kBlock - outIdx, effectiveRate, consumed, produced);
      }
      if (produced > 0) hasMore = true;
      int64_t newPos = pos + consumed;
      if (loop && newPos >= loopEnd) newPos = loopStart + (newPos - loopEnd);
      consumedThis += (newPos >= pos) ? (newPos - pos) : (loopEnd - pos + newPos - loopStart);
      pos = newPos;
      outIdx += produced;
      if (consumed == 0 && produced == 0) break;
    }
    st.pp += consumedThis;
  }
  if (loop && st.pp >= loopEnd) {  // :226-234, :349-357
    int64_t loopLength = loopEnd - loopStart;
    if (loopLength > 0) st.pp = loopStart + ((st.pp - loopEnd) % loopLength);
  }
  d.next = first < 0 ? 0 : first;
  d.produced = outIdx;
  end = !hasMore || (!loop && st.pp >= durEnd);
  return GSR_OK;
}

// Every index gsr_kernel will read for a descriptor that is not an END block: the window and the fed samples, walked with the
// kernel's own loop wrap rule.  A wrong descriptor must be an error, never a GPU fault.
__host__ __device__ inline int gsrCheckBlock(const GsrGeom& g, const GsrBlock& d) {
  int64_t ip = d.next;
  int64_t feeds = 0;
  if (d.copy) {
    feeds = d.produced;
  } else if (d.produced > 0) {
    for (int k = 0; k < 4; k++)
      if (d.w[k] < -1 || d.w[k] >= g.len) return GSR_ERR_WINDOW;
    feeds = 4 - d.ready;
    double P = d.pos;
    for (int o = 0; o < d.produced; o++) {
      int consume = (int)P;
      if (consume > 0) feeds += consume;
      P -= consume;
      P += d.rate;
    }
  }
  for (int64_t f = 0; f < feeds; f++) {
    if (ip < 0 || ip >= g.len) return GSR_ERR_FEED;
    ip++;
    if (g.loop && ip >= g.loopEnd) ip = g.loopStart;
  }
  return GSR_OK;
}

// ---- sources whose k-rate playbackRate is modulated by a signal (a two-stage chunk: Context::runChunkImpl) ----
// krate_probe_kernel: one lane per (param, block): clamp(intrinsic(t0) + mod[ch0][0], min, max), or the intrinsic value alone where the
// modulation input is silent (AudioParam.cs:143-165).  The rates stay on the device for gsr_walk_kernel and are read back by the host.
struct KrateProbeJob {
  uint64_t rows_off;     // plan offset of [nblocks] const float*: the mixed modulation input of each block (chunk-frame indexed), null = silent
  uint64_t events_off;   // plan offset of the parameter's events
  int nev;
  float value, vmin, vmax;
  int pad_;
  float* out;            // [nblocks] on the device
};
void launch_krate_probe(hipStream_t s, const KrateProbeJob* jobs_dev, int njobs, const uint8_t* plan_base_dev, const double* block_times_dev,
                        int64_t nblocks);

// gsr_walk_kernel: one lane per modulated buffer source walks the chunk's blocks in order (gsrReplayBlock) and writes the GsrBlock
// descriptors gsr_kernel consumes, plus a summary the host reads back.  Every index is checked here: a bad one sets `err` and its
// block's descriptor produces silence.
struct GsrWalkOut {
  int64_t endRel;   // first END block relative to the first played block, -1 = none
  GsrState st;      // after the walked blocks
  int err;          // GSR_* status of the first failure
  int pad_;
};
struct GsrWalkJob {
  GsrGeom g;
  GsrState st;            // at the first played block
  const float* rates;     // [nrates] k-rate values per chunk block (krate_probe_kernel)
  GsrBlock* desc;         // [nrel + 1]: one per walked block, then the state after them
  GsrWalkOut* out;
  int64_t bs, nrel;       // first played block (chunk relative), blocks to walk
  int64_t nrates;
  int endsAtEnd;          // stopTime is NaN: the first END block is the source's last (Ended, Dispose), the walk stops there
  int pad_;
};
void launch_gsr_walk(hipStream_t s, const GsrWalkJob* jobs_dev, int njobs);

}  // namespace ga
