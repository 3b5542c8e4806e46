// ga_conv_rebuild.hpp -- index arithmetic of the convolver migration (option "conv_migrate"): a node leaves formulation D
// for the B / C / R state layout and its spectra history is rebuilt from D's input history.  Plain C++: the kernel, the planner and
// the stand-alone host check (tests/conv_rebuild_main.cpp) share these functions.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GA_HD __host__ __device__
#else
#define GA_HD
#endif

namespace ga {

constexpr int kRebuildBlock = 128;   // = kBlock
constexpr int kRebuildBins = 129;    // = kBins

// One job = one input channel of one migrating node.  With T the first block of the migrating chunk and P the partition count,
// block j of the job (0 <= j < P) is block T - P + j of the channel.
struct ConvRebuildJob {
  const float* src;   // first sample of block T - P: P x 128 samples (nullptr: zeros)
  float* dst_r;       // [129][P - 1]: spectra of blocks T - P + 1 .. T - 1, the channel's part of ConvolverS::bHistR / bHistI
  float* dst_i;
  int P;
  int xrow;           // row of the scratch planes [row][129][tx] (ConvPlanesB) that receive blocks T - P .. T - 1
};

// D keeps the last `histLen` samples in front of the chunk: block T - P starts here (histLen = coarseP x 8192 >= P x 128)
GA_HD inline int64_t conv_rebuild_src_offset(int64_t histLen, int P) { return histLen - (int64_t)P * kRebuildBlock; }
// block j, 1 <= j < P, bin k -> element of the [129][P - 1] store
GA_HD inline size_t conv_rebuild_store_index(int P, int k, int j) { return (size_t)k * (size_t)(P - 1) + (size_t)(j - 1); }
// block j, 0 <= j < P, bin k -> element of the scratch planes: block T - 1 lies at column `hist` (where the forward transform of a
// one-block chunk would put it), the P - 1 blocks in front of it end at column hist - 1
GA_HD inline size_t conv_rebuild_plane_index(int xrow, int tx, int hist, int P, int k, int j) {
  return ((size_t)xrow * kRebuildBins + (size_t)k) * (size_t)tx + (size_t)(hist - (P - 1) + j);
}
// the scratch planes' geometry for the longest migrating node: `hist` columns in front of block T - 1 (16-byte aligned rows), four
// columns for the block itself (the partition sum writes and the inverse transform reads one aligned quad)
GA_HD inline int conv_rebuild_hist(int maxP) { return ((maxP - 1) + 3) / 4 * 4; }
GA_HD inline int conv_rebuild_tx(int maxP) { return conv_rebuild_hist(maxP) + 4; }
constexpr int kRebuildTy = 4;
// which input channel a slot reads: discrete -> slot c reads input c ; true stereo -> (L,h0) (L,h1) (R,h2) (R,h3)
GA_HD inline int conv_slot_input(bool trueStereo, int slot) { return trueStereo ? (slot >> 1) : slot; }

// The sets of a node on the B / C / R state layout: its slots (columns) grouped by the x-row they read, at most kConvSetCols per set
// (ConvSetB / ConvSetC).  For x-row xc = 0 .. nxr - 1 in turn, visit(xc, slots, ncol) receives the slots that read it, ascending, in
// runs of at most kConvSetCols; `shared`: the node's one x-row feeds every slot.  Nothing is allocated: a chunk plans a thousand nodes.
constexpr int kConvSetCols = 16;
template <class Visit>
inline void conv_for_each_set(bool shared, bool trueStereo, int nxr, int bSlots, Visit&& visit) {
  for (int xc = 0; xc < nxr; xc++) {
    int run[kConvSetCols], ncol = 0;
    for (int slot = 0; slot < bSlots; slot++) {
      if (!shared && conv_slot_input(trueStereo, slot) != xc) continue;
      run[ncol++] = slot;
      if (ncol == kConvSetCols) {
        visit(xc, (const int*)run, ncol);
        ncol = 0;
      }
    }
    if (ncol > 0) visit(xc, (const int*)run, ncol);
  }
}

}  // namespace ga
