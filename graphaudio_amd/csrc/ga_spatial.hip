// ga_spatial.hip -- SpatialPannerNode (DESIGN.md "SpatialPannerNode"): the binaural panner itself (spatial_panner_kernel), the
// built-in HRIR set (spatial_head_kernel, ga_spatial_head.hpp), the descriptors of signal-driven nodes (spatial_desc_kernel,
// ga_spatial_geom.hpp) and occlusion / three-band transmission (spatial_direct_kernel, ga_spatial_direct.hpp).  The node has no
// counterpart in the reference; the headers named here hold the arithmetic the host shares with the device.
// Wave64, -ffp-contract=off: see ga_kernels.hip.

#include "ga_kernels.hpp"
#include "ga_device_common.hpp"
#include "ga_fft16.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace ga {

// =====================================================================================================
//  SpatialPannerNode (DESIGN.md "SpatialPannerNode"): one workgroup = one node x a run of up to kSpatialRun blocks.
//    1. the mono mix m of the run's frames and of the T - 1 frames in front of them -> LDS (from the input views, or from the
//       node's carried history for frames in front of the chunk; silent blocks are zeros)
//    2. the run's filter pairs -> LDS: slot j belongs to block b0 - 1 + j (slot 0 only when block b0 fades from it); the HRIR
//       set is read here and nowhere else
//    3. one wavefront per block: lane l owns samples l and l + 64 and walks k = 0 .. T - 1 in pairs for both ears (and for the
//       previous block's pair while the block fades): per two taps, four reads of m (consecutive lanes, consecutive banks) and one
//       16-byte broadcast read per filter pair feed 8 fma (16 while fading) -- 5 LDS reads per 8 fma, 6 per 16
//  LDS: (kSpatialRun * 128 + 512) + (kSpatialRun + 1) * 2 * 512 floats = 24 KiB at T = 512 with a different filter in every
//  block: six workgroups per CU by LDS (160 KiB).  Every sum is the same chain whatever the run it falls into, so the output
//  does not depend on how a render is cut into chunks.
// =====================================================================================================
__device__ __forceinline__ float spatial_mix_at(const SpatialJob& job, const SpatialDesc* desc, const SpatialSeg* segs, int64_t f) {
  if (f < 0) return f >= -(int64_t)kSpatialMaxTaps ? gptr(job.hist_in)[kSpatialMaxTaps + f] : 0.f;
  const SpatialDesc* d = desc + 1 + (f >> 7);
  const int sg = d->seg;
  if (sg < 0) return 0.f;
  const SpatialSeg s = segs[sg];
  const float l = gptr(s.in_l)[f];
  if (d->flags & 2) return 0.5f * (l + gptr(s.in_r)[f]);
  return l;
}
__global__ __launch_bounds__(256) void spatial_panner_kernel(const SpatialWork* __restrict works, const SpatialJob* __restrict jobs,
                                                             const uint8_t* __restrict tables) {
  __shared__ float win[kSpatialRun * kBlock + kSpatialMaxTaps];
  __shared__ __attribute__((aligned(16))) float filt[kSpatialRun + 1][kSpatialMaxTaps][2];   // [slot][k][ear]: taps k, k + 1 of both ears are one 16-byte read
  const SpatialWork wk = works[blockIdx.x];
  const SpatialJob job = jobs[wk.job];
  const SpatialDesc* desc = (const SpatialDesc*)(tables + job.desc_off);
  const SpatialSeg* segs = (const SpatialSeg*)(tables + job.seg_off);
  const int tid = threadIdx.x;
  const int T = min(max(job.taps, 1), kSpatialMaxTaps);
  if (wk.tail) {   // the last kSpatialMaxTaps samples of m: the next chunk's history (the other copy: other workgroups still read hist_in)
    const int64_t N = job.nblocks * kBlock;
    for (int i = tid; i < kSpatialMaxTaps; i += 256) gptr(job.hist_out)[i] = spatial_mix_at(job, desc, segs, N - kSpatialMaxTaps + i);
  }
  const int nb = min(wk.nb, kSpatialRun);
  if (nb <= 0) return;
  const int64_t fA = (int64_t)wk.b0 * kBlock;
  const int nfr = nb * kBlock;
  for (int i = tid; i < nfr + T - 1; i += 256) win[i] = spatial_mix_at(job, desc, segs, fA - (T - 1) + i);   // win[i] = m[fA - (T - 1) + i]
  for (int j = 0; j <= nb; j++) {
    const SpatialDesc d = desc[wk.b0 + j];   // (table entry b + 1 = block b: slot j = block b0 - 1 + j)
    if (j == 0 && !(desc[wk.b0 + 1].flags & 1)) continue;
    if (j > 0 && d.seg < 0) continue;        // a silent block renders nothing, and the block after it does not fade
    for (int e = tid; e < 2 * T; e += 256) {
      const int ear = e >= T ? 1 : 0, k = e - ear * T;
      float acc = 0.f;
#pragma unroll
      for (int q = 0; q < 4; q++) acc = fmaf(d.w[q], gptr(job.hrir)[(int64_t)(2 * d.idx[q] + ear) * job.hstride + k], acc);
      filt[j][k][ear] = d.gb * acc;
    }
  }
  __syncthreads();
  // One wavefront per block of the run; lane l owns samples l and l + 64 of its block, which share the block's filters: per pair of
  // taps one 16-byte broadcast read per filter pair and four conflict-free reads of m feed 8 fma (16 while the block fades).
  const int bl = tid >> 6, lane = tid & 63;
  if (bl >= nb) return;
  const SpatialDesc d = desc[wk.b0 + 1 + bl];
  if (d.seg < 0) return;
  const bool fade = (d.flags & 1) != 0;
  const float* w0 = win + (T - 1) + bl * kBlock + lane;   // w0[-k] = m[n - k] for sample n = lane; w0[64 - k] for sample lane + 64
  const f32x4* fc = (const f32x4*)&filt[bl + 1][0][0];
  const f32x4* fp = (const f32x4*)&filt[bl][0][0];
  float cl0 = 0.f, cr0 = 0.f, cl1 = 0.f, cr1 = 0.f, pl0 = 0.f, pr0 = 0.f, pl1 = 0.f, pr1 = 0.f;
  const int T2 = T & ~1;
  if (fade) {
#pragma unroll 2
    for (int k = 0; k < T2; k += 2) {
      const f32x4 c = fc[k >> 1], p = fp[k >> 1];
      const float a0 = w0[-k], a1 = w0[-k - 1], b0 = w0[64 - k], b1 = w0[63 - k];
      cl0 = fmaf(c.x, a0, cl0); cr0 = fmaf(c.y, a0, cr0); pl0 = fmaf(p.x, a0, pl0); pr0 = fmaf(p.y, a0, pr0);
      cl1 = fmaf(c.x, b0, cl1); cr1 = fmaf(c.y, b0, cr1); pl1 = fmaf(p.x, b0, pl1); pr1 = fmaf(p.y, b0, pr1);
      cl0 = fmaf(c.z, a1, cl0); cr0 = fmaf(c.w, a1, cr0); pl0 = fmaf(p.z, a1, pl0); pr0 = fmaf(p.w, a1, pr0);
      cl1 = fmaf(c.z, b1, cl1); cr1 = fmaf(c.w, b1, cr1); pl1 = fmaf(p.z, b1, pl1); pr1 = fmaf(p.w, b1, pr1);
    }
  } else {
#pragma unroll 2
    for (int k = 0; k < T2; k += 2) {
      const f32x4 c = fc[k >> 1];
      const float a0 = w0[-k], a1 = w0[-k - 1], b0 = w0[64 - k], b1 = w0[63 - k];
      cl0 = fmaf(c.x, a0, cl0); cr0 = fmaf(c.y, a0, cr0);
      cl1 = fmaf(c.x, b0, cl1); cr1 = fmaf(c.y, b0, cr1);
      cl0 = fmaf(c.z, a1, cl0); cr0 = fmaf(c.w, a1, cr0);
      cl1 = fmaf(c.z, b1, cl1); cr1 = fmaf(c.w, b1, cr1);
    }
  }
  if (T2 < T) {   // an odd T: the last tap on its own (the pair read would look one sample in front of the staged window)
    const int k = T2;
    const float a0 = w0[-k], b0 = w0[64 - k];
    const float l = filt[bl + 1][k][0], r = filt[bl + 1][k][1];
    cl0 = fmaf(l, a0, cl0); cr0 = fmaf(r, a0, cr0); cl1 = fmaf(l, b0, cl1); cr1 = fmaf(r, b0, cr1);
    if (fade) {
      const float ql = filt[bl][k][0], qr = filt[bl][k][1];
      pl0 = fmaf(ql, a0, pl0); pr0 = fmaf(qr, a0, pr0); pl1 = fmaf(ql, b0, pl1); pr1 = fmaf(qr, b0, pr1);
    }
  }
  const SpatialSeg sg = segs[d.seg];
  const float pdry = fade ? desc[wk.b0 + bl].dry : 0.f;
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const int n = lane + 64 * h;
    const int64_t f = fA + bl * kBlock + n;
    const float xl = gptr(sg.in_l)[f];
    const float xr = (d.flags & 2) ? gptr(sg.in_r)[f] : xl;
    float yl = fmaf(d.dry, xl, h ? cl1 : cl0), yr = fmaf(d.dry, xr, h ? cr1 : cr0);
    if (fade) {
      const float wn = (float)(n + 1) * (1.0f / kBlock);
      yl = fmaf(wn, yl, (1.0f - wn) * fmaf(pdry, xl, h ? pl1 : pl0));
      yr = fmaf(wn, yr, (1.0f - wn) * fmaf(pdry, xr, h ? pr1 : pr0));
    }
    gptr(job.out_l)[f] = yl;
    gptr(job.out_r)[f] = yr;
  }
}
void launch_spatial_panner(hipStream_t s, const SpatialWork* works_dev, int nworks, const SpatialJob* jobs_dev, const uint8_t* tables_dev) {
  if (nworks <= 0) return;
  hipLaunchKernelGGL(spatial_panner_kernel, dim3(nworks), dim3(256), 0, s, works_dev, jobs_dev, tables_dev);
}

// ======================================================================================================
//  The built-in HRIR set (ga_spatial_head.hpp): workgroup = channel (one wavefront), lane = tap k, k + 64, ...  Every lane works out
//  its channel's delay and shadow filter for itself and sums its tap's (at most 16) products in double: no lane reads what another
//  wrote, no LDS.  Runs once per set and sample rate / head radius, so nothing here is tuned: 3600 x T taps of ~16 terms each.
// ======================================================================================================
__global__ __launch_bounds__(64) void spatial_head_kernel(float* __restrict out, int64_t stride, int taps, double fs, double a) {
  const int ch = blockIdx.x;   // (the grid is 2 * kSpatialHeadDirs workgroups: launch_spatial_head)
  const SpatialHeadEar e = spatial_head_ear(fs, a, ch);
  for (int k = threadIdx.x; k < taps; k += 64) gptr(out)[(int64_t)ch * stride + k] = spatial_head_tap(e, k);
}
void launch_spatial_head(hipStream_t s, float* out, int64_t stride, int taps, double fs, double a) {
  if (taps < 1 || taps > kSpatialMaxTaps || stride < taps) launch_fail("spatial_head_kernel: taps / stride");
  hipLaunchKernelGGL(spatial_head_kernel, dim3(2 * kSpatialHeadDirs), dim3(64), 0, s, out, stride, taps, fs, a);
}

// ======================================================================================================
//  SpatialPannerNode descriptors of signal-driven nodes (ga_kernels.hpp, SpatialDescJob): one lane per (node, block), wave64.
//  A lane depends on no other lane of the launch: the previous block's geometry, which decides the fade, is recomputed from that
//  block's inputs (blocks b0 + 1 ..), or read from the carried descriptor an earlier launch or the host left (block b0).
//  The job is read through the uniform pointer (scalar loads), the parameter loops are unrolled: no scratch.
// ======================================================================================================
__device__ __forceinline__ void spatial_desc_geometry(const SpatialDescJob& job, const uint8_t* tables, const SpatialListener& L, int b, SpatialGeom& o, SpatialEq& eq) {
  float pv[kSpatialParams];
#pragma unroll
  for (int p = 0; p < kSpatialParams; p++) {
    float v = job.curve_off[p] != kSpatialNoCurve ? gptr((const float*)(tables + job.curve_off[p]))[b] : job.value[p];
    const float* m = job.mod[p];
    if (m) v = clamp_ref(v + gptr(m)[(int64_t)b * kBlock], job.vmin[p], job.vmax[p]);   // Math.Clamp(intrinsicValue + modulation, min, max), sample 0
    pv[p] = v;
  }
  spatial_geometry<SpatialMathDouble>(pv, L.v, job.model, job.azimuths, job.dirs, o);
  if (job.eq_off != kSpatialNoCurve) {   // option "spatial_occlusion": the largest band factor joins g, the rest is the block's EQ triple
    float s;
    spatial_occlusion(pv[13], pv[14], pv[15], pv[16], s, eq);
    o.g = o.g * s;
  }
}
__global__ __launch_bounds__(64) void spatial_desc_kernel(const SpatialDescJob* __restrict jobs, uint8_t* __restrict tables, SpatialListener L) {
  const SpatialDescJob& job = jobs[blockIdx.y];
  const int i = (int)(blockIdx.x * 64 + threadIdx.x);
  if (i >= job.nb) return;
  const int b = job.b0 + i;
  GA_GLOBAL SpatialDesc* desc = gptr((SpatialDesc*)(tables + job.desc_off));
  const int dmax = max(job.dirs, 1) - 1;
  SpatialGeom cur, pr;
  SpatialEq eq{1.0f, 0.0f, 0.0f}, eqPr;
  spatial_desc_geometry(job, tables, L, b, cur, eq);
  bool have = false;
  if (i > 0) {
    spatial_desc_geometry(job, tables, L, b - 1, pr, eqPr);
    have = true;
  } else if (job.prev_valid) {
    SpatialCarry c = job.prev_host;
    if (job.prev_in) {
      const GA_GLOBAL SpatialCarry* pc = gptr(job.prev_in);
      for (int q = 0; q < 4; q++) {
        c.idx[q] = pc->idx[q];
        c.w[q] = pc->w[q];
      }
      c.g = pc->g;
      c.beta = pc->beta;
    }
    for (int q = 0; q < 4; q++) {
      pr.idx[q] = c.idx[q];
      pr.w[q] = c.w[q];
    }
    pr.g = c.g;
    pr.beta = c.beta;
    have = true;
    if (b == 0 && job.prev_in) {   // entry 0, the block in front of the chunk (the host wrote it where it holds the descriptor)
      for (int q = 0; q < 4; q++) {
        desc[0].idx[q] = min(max(pr.idx[q], 0), dmax);
        desc[0].w[q] = pr.w[q];
      }
      desc[0].gb = pr.g * pr.beta;
      desc[0].dry = pr.g * (1.0f - pr.beta);
    }
  }
  const bool fade = have && spatial_differs(pr, cur);
  GA_GLOBAL SpatialDesc* d = desc + b + 1;
  for (int q = 0; q < 4; q++) {
    d->idx[q] = min(max(cur.idx[q], 0), dmax);
    d->w[q] = cur.w[q];
  }
  d->gb = cur.g * cur.beta;
  d->dry = cur.g * (1.0f - cur.beta);
  d->flags = (d->flags & ~1) | (fade ? 1 : 0);
  if (job.eq_off != kSpatialNoCurve) {
    GA_GLOBAL SpatialEqEntry* e = gptr((SpatialEqEntry*)(tables + job.eq_off)) + b + 1;
    e->c.cM = eq.cM;
    e->c.cL = eq.cL;
    e->c.cH = eq.cH;
  }
  if (i == job.nb - 1) {
    GA_GLOBAL SpatialCarry* po = gptr(job.prev_out);
    for (int q = 0; q < 4; q++) {
      po->idx[q] = cur.idx[q];
      po->w[q] = cur.w[q];
    }
    po->g = cur.g;
    po->beta = cur.beta;
  }
}
void launch_spatial_desc(hipStream_t s, const SpatialDescJob* jobs_dev, int njobs, int max_nb, uint8_t* tables_dev, const SpatialListener& listener) {
  if (njobs <= 0 || max_nb <= 0) return;
  const int gx = (max_nb + 63) / 64;
  GA_LAUNCH_JOBS(spatial_desc_kernel, gx, 64, jobs_dev, njobs, tables_dev, listener);
}

// ======================================================================================================
//  SpatialPannerNode occlusion / three-band transmission (ga_kernels.hpp, SpatialDirectJob; DESIGN.md "SpatialPannerNode",
//  "Occlusion and transmission"): x' of every input channel in front of spatial_panner_kernel.  One lane per (node, channel)
//  walks the chunk's blocks in time order with both one-pole recurrences in registers -- serial in time on purpose: every sample
//  is the same chain however the render is cut into chunks; nodes and channels are the parallel axis.  One wavefront per
//  workgroup serves kSpatialDirectRows rows (8 nodes): few rows per wave, because the walk is latency bound and a level of a
//  thousand nodes should reach every CU.  Per block the wave stages its rows' 128 frames through a [16][129] LDS tile in both
//  directions (row r is read and written by all 64 lanes at consecutive addresses; lane l < 16 then walks tile[l][.], bank
//  (l + n) mod 64: no conflict), so no lane walks its own global row.  A block that is not active passes through the tile unchanged.
// ======================================================================================================
constexpr int kSpatialDirectRows = 16;   // (node, channel) rows per wavefront
__global__ __launch_bounds__(64) void spatial_direct_kernel(const SpatialDirectJob* __restrict jobs, int njobs, int max_nb,
                                                            const uint8_t* __restrict tables, SpatialBands K) {
  __shared__ float tile[kSpatialDirectRows][kBlock + 1];
  __shared__ const float* src[kSpatialDirectRows];
  __shared__ float* dst[kSpatialDirectRows];
  const int lane = threadIdx.x, ch = lane & 1;
  const int ji = (int)blockIdx.x * (kSpatialDirectRows / 2) + (lane >> 1);
  const bool mine = lane < kSpatialDirectRows && ji < njobs;
  const SpatialDirectJob& job = jobs[mine ? ji : 0];
  const float* const inp = job.in[ch];
  float* const outp = job.out[ch];
  const bool walks = mine && inp != nullptr;   // (lane 1 of a mono segment has nothing to do: its run is not open afterwards)
  const int nb = walks ? job.nb : 0;
  const int64_t fA = (int64_t)job.b0 * kBlock;
  const GA_GLOBAL SpatialEqEntry* eqs = gptr((const SpatialEqEntry*)(tables + job.eq_off)) + job.b0 + 1;
  GA_GLOBAL SpatialDirectState* st = gptr(job.state);
  float zl = 0.f, zh = 0.f;
  SpatialEq pr{1.0f, 0.0f, 0.0f};
  bool have = false, open = false;
  if (walks) {
    have = job.prev_valid != 0;
    if (job.from_state) {
      pr.cM = st->prev.cM;
      pr.cL = st->prev.cL;
      pr.cH = st->prev.cH;
      open = st->open[ch] != 0;
    } else {
      pr = job.prev;
      open = ((job.open >> ch) & 1) != 0;
    }
    open = open && have;
    if (open) {
      zl = st->zl[ch];
      zh = st->zh[ch];
    }
  }
  for (int b = 0; b < max_nb; b++) {
    const bool on = b < nb;
    if (lane < kSpatialDirectRows) {
      src[lane] = on ? inp + fA + (int64_t)b * kBlock : nullptr;
      dst[lane] = on ? outp + fA + (int64_t)b * kBlock : nullptr;
    }
    __syncthreads();
#pragma unroll 4
    for (int r = 0; r < kSpatialDirectRows; r++) {
      const float* p = src[r];
      if (p) {
        tile[r][lane] = gptr(p)[lane];
        tile[r][64 + lane] = gptr(p)[64 + lane];
      }
    }
    __syncthreads();
    if (on) {
      SpatialEq cur;
      cur.cM = eqs[b].c.cM;
      cur.cL = eqs[b].c.cL;
      cur.cH = eqs[b].c.cH;
      if (!have) pr = cur;   // the first processed block after creation or silence: its own triple alone
      const bool active = !spatial_eq_identity(cur) || !spatial_eq_identity(pr);
      if (active) {
        if (!open) zl = zh = 0.f;   // the first block of a run of active blocks
#pragma unroll 8
        for (int n = 0; n < kBlock; n++) tile[lane][n] = spatial_direct_step(K, spatial_eq_at(pr, cur, n), tile[lane][n], zl, zh);
      }
      open = active;
      have = true;
      pr = cur;
    }
    __syncthreads();
#pragma unroll 4
    for (int r = 0; r < kSpatialDirectRows; r++) {
      float* p = dst[r];
      if (p) {
        gptr(p)[lane] = tile[r][lane];
        gptr(p)[64 + lane] = tile[r][64 + lane];
      }
    }
    __syncthreads();
  }
  if (mine) {
    st->zl[ch] = zl;
    st->zh[ch] = zh;
    st->open[ch] = (walks && open) ? 1 : 0;
    if (ch == 0) {
      st->prev.cM = pr.cM;
      st->prev.cL = pr.cL;
      st->prev.cH = pr.cH;
    }
  }
}
void launch_spatial_direct(hipStream_t s, const SpatialDirectJob* jobs_dev, int njobs, int max_nb, const uint8_t* tables_dev, const SpatialBands& bands) {
  if (njobs <= 0 || max_nb <= 0) return;
  const int per = kSpatialDirectRows / 2;
  hipLaunchKernelGGL(spatial_direct_kernel, dim3((njobs + per - 1) / per), dim3(64), 0, s, jobs_dev, njobs, max_nb, tables_dev, bands);
}

}  // namespace ga
