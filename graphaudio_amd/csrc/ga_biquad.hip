// ga_biquad.hip -- BiQuadFilterNode (BiQuadFilterNode.cs): constant coefficients as one lane per cascade (biquad_kernel,
// biquad1_kernel), as a software pipeline across lanes in inline assembly (biquad_pipe_kernel, ga_biquad_pipe_asm.inc) and split
// in time (biquad_split_expand_kernel, biquad_scan_kernel, ga_biquad_split.hpp); automated coefficients in
// biquad_dynamic_kernel.  Every path keeps the reference's sample-by-sample float32 arithmetic.  tools/micro/bq_pipe_probe.hip and
// bq_pipe_check.hip include this file whole.  Wave64, 64x64 tiles through LDS, -ffp-contract=off: see ga_kernels.hip.

#include "ga_kernels.hpp"
#include "ga_fft16.hpp"
#include "ga_libmf.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

namespace ga {

// =====================================================================================================
//  BiQuadFilterNode with constant coefficients (BiQuadFilterNode.cs:136-141): one lane per (node, channel),
//  64 jobs per wavefront.  The wave stages a [64 jobs][64 frames] tile through LDS so every HBM access is a
//  coalesced 256-byte row even though each lane walks its own slab serially.
// =====================================================================================================
constexpr int BQ_TILE = 64;
__device__ __forceinline__ const float* bcast_ptr(const float* p, int srcLane) {
  unsigned long long v = (unsigned long long)p;
  unsigned lo = __builtin_amdgcn_readlane((unsigned)v, srcLane), hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), srcLane);
  return (const float*)(((unsigned long long)hi << 32) | lo);
}
// JPW = cascades (jobs) per wavefront.  The recurrence is latency/issue bound, not lane bound: with few jobs it is far
// better to spread them thinly (4..16 lanes busy per wave, every SIMD of the chip working) than to fill 64 lanes of a
// handful of waves.  All 64 lanes still cooperate on the coalesced 256-byte row loads / stores of the JPW x 64 tile.
template <int NSEC, int JPW>
__global__ __launch_bounds__(64) void biquad_kernel(const BiquadJob* __restrict jobs, int njobs, const BiquadSection* __restrict secs) {
  // tile length: long tiles amortise the load / barrier / store overhead of a tile when few chains share a wavefront
  constexpr int TL = JPW <= 8 ? 256 : BQ_TILE, TM = TL / 64;
  __shared__ float tile[JPW][TL + 1];
  __shared__ float prevw[JPW][2];   // NSEC == 1: W1, W2 at the start of the tile (the FIR half needs w[-1], w[-2])
  const int lane = threadIdx.x;
  const int j0 = blockIdx.x * JPW;
  const int myj = j0 + lane;
  const bool have = lane < JPW && myj < njobs;
  // every compute lane keeps ITS job (cascade coefficients and states) in registers; row pointers are broadcast with v_readlane
  BiquadJob me{};
  if (have) me = jobs[myj];
  const float* inb = have ? me.in + me.f0 : nullptr;
  float* outb = (have && me.out) ? me.out + me.f0 : nullptr;
  float b0[NSEC], b1[NSEC], b2[NSEC], a1[NSEC], a2[NSEC], w1[NSEC], w2[NSEC];
  float* st[NSEC];
#pragma unroll
  for (int q = 0; q < NSEC; q++) {
    b0[q] = b1[q] = b2[q] = a1[q] = a2[q] = w1[q] = w2[q] = 0.f;
    st[q] = nullptr;
    if (have) {
      const BiquadSection sc = secs[me.sec0 + q];
      b0[q] = sc.b0; b1[q] = sc.b1; b2[q] = sc.b2; a1[q] = sc.a1; a2[q] = sc.a2;
      st[q] = me.state ? me.state + 2 * q : sc.state;
      w1[q] = ldg1(st[q]);
      w2[q] = ldg1(st[q] + 1);
    }
  }
  const int64_t n = have ? me.n : 0;
  int64_t nmax = n;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) nmax = max(nmax, (int64_t)__shfl_xor((long long)nmax, m, 64));
  const int jcount = min(JPW, njobs - j0);

  float pre[JPW][TM];   // prefetched tile: pre[r][u] = frame (base + 64 u + lane) of job j0 + r
  auto fetch = [&](int64_t base) {
#pragma unroll
    for (int r = 0; r < JPW; r++) {
      const float* p = bcast_ptr(inb, r);
      int64_t nr = __builtin_amdgcn_readlane((int)n, r);   // n < 2^31 frames per segment
#pragma unroll
      for (int u = 0; u < TM; u++) {
        int64_t fi = base + 64 * u + lane;
        pre[r][u] = (r < jcount && fi < nr) ? ldg1(p + fi) : 0.f;
      }
    }
  };
  fetch(0);
  for (int64_t base = 0; base < nmax; base += TL) {
#pragma unroll
    for (int r = 0; r < JPW; r++)
#pragma unroll
      for (int u = 0; u < TM; u++) tile[r][64 * u + lane] = pre[r][u];
    __syncthreads();
    if (base + TL < nmax) fetch(base + TL);   // next tile's loads fly during the serial recurrence below
    const int cnt = (int)max<int64_t>(0, min<int64_t>(TL, n - base));
    if constexpr (NSEC == 1) {
      // A single section splits into a RECURSIVE half  w[n] = x[n] - a1 w[n-1] - a2 w[n-2]  (serial, one lane per chain) and a
      // FIR half  y[n] = b0 w[n] + b1 w[n-1] + b2 w[n-2]  (no recurrence: all 64 lanes, one sample each).  The same products
      // and sums in the same order as BiQuadFilterNode.cs:137-138 -> bit-exact, with 4 instead of 9 flops on the serial chain.
      if (lane < JPW) {
        prevw[lane][0] = w1[0];
        prevw[lane][1] = w2[0];
        float ww1 = w1[0], ww2 = w2[0];
        const float ca1 = a1[0], ca2 = a2[0];
        // the chain  a1 w1 -> (x - .) -> (. - a2 w2)  is three dependent VALU results per sample (~20 cycles each on gfx950): keep
        // everything else -- the select of a partial tile included -- off it
        if (cnt == TL) {
#pragma unroll
          for (int i0 = 0; i0 < TL; i0 += 16) {
            float xv[16];
#pragma unroll
            for (int i = 0; i < 16; i++) xv[i] = tile[lane][i0 + i];
#pragma unroll
            for (int i = 0; i < 16; i++) {
              const float w = xv[i] - ca1 * ww1 - ca2 * ww2;
              ww2 = ww1;
              ww1 = w;
              xv[i] = w;
            }
#pragma unroll
            for (int i = 0; i < 16; i++) tile[lane][i0 + i] = xv[i];
          }
        } else {
          for (int i = 0; i < cnt; i++) {
            const float w = tile[lane][i] - ca1 * ww1 - ca2 * ww2;
            ww2 = ww1;
            ww1 = w;
            tile[lane][i] = w;
          }
        }
        w1[0] = ww1;
        w2[0] = ww2;
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < JPW; r++) {
        if (r < jcount) {
          const float cb0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b0[0]), r));
          const float cb1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b1[0]), r));
          const float cb2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b2[0]), r));
          float yv[TM];
#pragma unroll
          for (int u = 0; u < TM; u++) {
            const int x = 64 * u + lane;
            const float w0 = tile[r][x];
            const float wm1 = x >= 1 ? tile[r][x - 1] : prevw[r][0];
            const float wm2 = x >= 2 ? tile[r][x - 2] : prevw[r][1 - x];   // x = 1: w[-1] ; x = 0: w[-2]
            yv[u] = cb0 * w0 + cb1 * wm1 + cb2 * wm2;
          }
          // (one wavefront: its LDS reads above are served before the writes below)
#pragma unroll
          for (int u = 0; u < TM; u++) tile[r][64 * u + lane] = yv[u];
        }
      }
    } else if (lane < JPW) {
      if (cnt == TL) {
        // register batches of 16 keep LDS latency off the W1/W2 dependency chains
#pragma unroll
        for (int i0 = 0; i0 < TL; i0 += 16) {
          float xv[16];
#pragma unroll
          for (int i = 0; i < 16; i++) xv[i] = tile[lane][i0 + i];
#pragma unroll
          for (int i = 0; i < 16; i++) {
            float x = xv[i];
#pragma unroll
            for (int q = 0; q < NSEC; q++) {
              float w = x - a1[q] * w1[q] - a2[q] * w2[q];            // BiQuadFilterNode.cs:137
              float y = b0[q] * w + b1[q] * w1[q] + b2[q] * w2[q];    // :138
              w2[q] = w1[q];
              w1[q] = w;
              x = y;
            }
            xv[i] = x;
          }
#pragma unroll
          for (int i = 0; i < 16; i++) tile[lane][i0 + i] = xv[i];
        }
      } else {
        for (int i = 0; i < cnt; i++) {   // the job's last, partial tile
          float x = tile[lane][i];
#pragma unroll
          for (int q = 0; q < NSEC; q++) {
            float w = x - a1[q] * w1[q] - a2[q] * w2[q];
            float y = b0[q] * w + b1[q] * w1[q] + b2[q] * w2[q];
            w2[q] = w1[q];
            w1[q] = w;
            x = y;
          }
          tile[lane][i] = x;
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < JPW; r++) {
      if (r < jcount) {
        float* q = (float*)bcast_ptr(outb, r);
        if (!q) continue;   // (a state-only job: pass A of a cascade split along time)
        int64_t nr = __builtin_amdgcn_readlane((int)n, r);
#pragma unroll
        for (int u = 0; u < TM; u++) {
          int64_t fi = base + 64 * u + lane;
          if (fi < nr) stg1(q + fi, tile[r][64 * u + lane]);
        }
      }
    }
    __syncthreads();
  }
  if (have) {
#pragma unroll
    for (int q = 0; q < NSEC; q++)
      for (int t = 0; t < me.twins; t++) {   // (twin channels: BiquadJob::twins)
        stg1(st[q] + 2 * t, w1[q]);
        stg1(st[q] + 2 * t + 1, w2[q]);
      }
  }
}
template <int JPW>
static void launch_biquad_jpw(hipStream_t s, const BiquadJob* jobs_dev, int njobs, const BiquadSection* secs_dev, int nsec) {
  dim3 g((njobs + JPW - 1) / JPW), b(64);
  switch (nsec) {
    case 1: hipLaunchKernelGGL((biquad_kernel<1, JPW>), g, b, 0, s, jobs_dev, njobs, secs_dev); break;
    case 2: hipLaunchKernelGGL((biquad_kernel<2, JPW>), g, b, 0, s, jobs_dev, njobs, secs_dev); break;
    case 3: hipLaunchKernelGGL((biquad_kernel<3, JPW>), g, b, 0, s, jobs_dev, njobs, secs_dev); break;
    case 4: hipLaunchKernelGGL((biquad_kernel<4, JPW>), g, b, 0, s, jobs_dev, njobs, secs_dev); break;
    case 5: hipLaunchKernelGGL((biquad_kernel<5, JPW>), g, b, 0, s, jobs_dev, njobs, secs_dev); break;
    case 6: hipLaunchKernelGGL((biquad_kernel<6, JPW>), g, b, 0, s, jobs_dev, njobs, secs_dev); break;
    case 7: hipLaunchKernelGGL((biquad_kernel<7, JPW>), g, b, 0, s, jobs_dev, njobs, secs_dev); break;
    default: hipLaunchKernelGGL((biquad_kernel<8, JPW>), g, b, 0, s, jobs_dev, njobs, secs_dev); break;
  }
}
// ---- cascades of NSEC >= 2 sections: the sections of one cascade sit on NEIGHBOURING LANES -----------------------------------
// Lane q of a group runs section q on sample k - SK q at step k and takes its input from lane q - 1 with one DPP row shift: a
// software pipeline across lanes.  Per step the wave issues ONE section's arithmetic instead of NSEC sections back to back on
// a single lane; every section still sees exactly the reference's sample-by-sample float arithmetic
// (BiQuadFilterNode.cs:137-138: w = (x - a1 w1) - a2 w2 ; y = (b0 w + b1 w1) + b2 w2), so the result stays bit-exact.
// 16 / NSEC cascades per 16-lane row.
//
// A wave that is alone on its SIMD pays ~5 cycles per instruction, whatever the instruction (vector, scalar, s_nop, LDS; measured with
// tools/micro/bq_pipe_probe.hip: 221 instructions per 16 steps = 1131 cycles), and ~4 more when it needs the result of the
// instruction right before it: the walk costs its instruction COUNT.  Its steady state is therefore ONE inline-assembly
// statement with fixed registers (ga_biquad_pipe_asm.inc, written by tools/gen_biquad_pipe_asm.py, where the schedule is
// described): 8 vector instructions per step --
//   the four products of w[k-1] as two packed multiplies ({a1, b1} w and {a2, b2} w: P1, R1 of this step, P2, R2 of the next);
//   the recursion  t = x - P1 ; w = t - P2 ;
//   the output half (m = b0 w ; s = m + R1 ; y = s + R2) one and two steps behind, in the gaps of the recursion;
//   the hand-over from the lane to the left and the select of the cascade's input for section 0 as one v_cndmask_b32_dpp
// -- plus one instruction per step for the LDS traffic and the loop; no instruction follows its producer.  SK = 4 steps between
// neighbouring sections keep the hand-over off the dependency chain.  The pipeline is filled once per JOB and drained once
// (masked batches, plain C++), not per tile: step k hands out sample k - D, D = SK (NSEC - 1), the tile is stored D samples late.
#ifdef GA_BQ_PROBE   // tools/micro/bq_pipe_probe.hip: where a wave's cycles go (s_memtime around the phases of every tile)
__device__ unsigned long long ga_bq_probe[8];
}   // namespace ga
// (a library built with -DGA_BQ_PROBE hands the sums out and clears them: tools/bq_probe_product.py)
extern "C" __attribute__((visibility("default"))) void ga_bq_probe_read(unsigned long long* out) {
  unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(ga::ga_bq_probe), sizeof zero);
  (void)hipMemcpyToSymbol(HIP_SYMBOL(ga::ga_bq_probe), zero, sizeof zero);
}
namespace ga {
#define GA_BQ_T(v) const unsigned long long v = __builtin_amdgcn_s_memtime()
#define GA_BQ_ACC(i, v) probe_acc[i] += (v)
#else
#define GA_BQ_T(v)
#define GA_BQ_ACC(i, v)
#endif
template <int NSEC>
__global__ __launch_bounds__(64) void biquad_pipe_kernel(const BiquadJob* __restrict jobs, int njobs, const BiquadSection* __restrict secs,
                                                         int jpw) {
  constexpr int GPR = 16 / NSEC;        // cascades (groups of NSEC lanes) per row
  constexpr int MAXJ = 4 * GPR < 16 ? 4 * GPR : 16;   // (16: the tile's rows live in registers twice, prefetched and outgoing)
  constexpr int PT = 256, TM = PT / 64;   // steps per tile
  constexpr int SK = 4;                   // steps between a section and the next
  constexpr int D = SK * (NSEC - 1);      // step k hands out sample k - D
  constexpr int LD = PT + 4;              // 16-byte aligned rows: a batch of 16 steps reads / writes its samples as four b128
  __shared__ __attribute__((aligned(16))) float tile[MAXJ][LD];
  __shared__ __attribute__((aligned(16))) float dump[64][16];   // where the lanes that are not a last section "write their outputs"
  const int lane = threadIdx.x;
  const int row = lane >> 4, lr = lane & 15;
  const int grp = lr / NSEC, q = lr % NSEC;
  const int slot = row * GPR + grp;                       // cascade slot of this lane inside the wave
  const int j0 = blockIdx.x * jpw;
  const int myj = j0 + slot;
  const bool have = grp < GPR && slot < jpw && myj < njobs;
  BiquadJob me{};
  if (have) me = jobs[myj];
  const float* inb = have ? me.in + me.f0 : nullptr;
  float* outb = have ? me.out + me.f0 : nullptr;
  float b0 = 0.f, w1 = 0.f, w2 = 0.f, w3 = 0.f;   // w3: the w before w2 (for the assembly walk to pick up mid-stream; not state)
  v2f ab1 = {0.f, 0.f}, ab2 = {0.f, 0.f};   // {a1, b1}, {a2, b2}
  float* st = nullptr;
  if (have) {
    const BiquadSection sc = secs[me.sec0 + q];
    b0 = sc.b0;
    ab1 = v2f{sc.a1, sc.b1};
    ab2 = v2f{sc.a2, sc.b2};
    st = me.state ? me.state + 2 * q : sc.state;
    w1 = ldg1(st);
    w2 = ldg1(st + 1);
  }
  const int n = have ? (int)me.n : 0;
  int nmax = n, nmin = have ? n : 0x7fffffff;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    nmax = max(nmax, __shfl_xor(nmax, m, 64));
    nmin = min(nmin, __shfl_xor(nmin, m, 64));
  }
  nmax = __builtin_amdgcn_readfirstlane(nmax);
  nmin = __builtin_amdgcn_readfirstlane(nmin);
  const int jcount = min(jpw, njobs - j0);
  auto lane_of = [](int r) { return (r / GPR) * 16 + (r % GPR) * NSEC; };   // lane of section 0 of slot r

  // A tile row in flight (prefetched / outgoing) is four registers per lane, in one of two layouts:
  //   whole tiles   lane l holds frames 4 l .. 4 l + 3 of the row: ONE 16-byte global access and one b128 LDS access per row
  //   ragged tiles  register u holds frame 64 u + l, every access bounds-checked (a job's first and last tiles)
  v4f pre[MAXJ];
  bool pre_whole = false;
  auto fetch = [&](int base) {
    pre_whole = base + PT <= nmin;
    if (pre_whole) {
#pragma unroll
      for (int r = 0; r < MAXJ; r++)
        if (r < jcount) pre[r] = ldg4(bcast_ptr(inb, lane_of(r)) + base + 4 * lane);
      return;
    }
#pragma unroll
    for (int r = 0; r < MAXJ; r++) {
      pre[r] = v4f{0.f, 0.f, 0.f, 0.f};
      if (r < jcount) {
        const float* p = bcast_ptr(inb, lane_of(r));
        const int nr = __builtin_amdgcn_readlane(n, lane_of(r));
#pragma unroll
        for (int u = 0; u < TM; u++) {
          const int fi = base + 64 * u + lane;
          if (fi < nr) pre[r][u] = ldg1(p + fi);
        }
      }
    }
  };
  const int srow = have ? slot : 0;
  const bool q0 = q == 0;
  const bool qlast = have && q == NSEC - 1;
  const int jofs = SK * q;
  float yh[SK];   // this lane's outputs of the last SK steps, yh[0] the latest
#pragma unroll
  for (int i = 0; i < SK; i++) yh[i] = 0.f;
  auto dpp_left = [](float v) {   // lane l takes lane l - 1's value (row_shr:1); a row's lane 0 is always a section 0
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xF, 0xF, false));
  };
  // nb batches of 16 steps in which every section of every cascade of the wave has a sample (tile positions p0 ...)
  const unsigned long long q0mask = __builtin_amdgcn_ballot_w64(q0);
  auto steady_run = [&](int p0, int nb) {
    typedef __attribute__((address_space(3))) float* lds_ptr;   // (a 32-bit LDS offset: what ds_read / ds_write address)
    const unsigned ain = (unsigned)(size_t)(lds_ptr)&tile[srow][p0];
    const unsigned aout = qlast ? ain : (unsigned)(size_t)(lds_ptr)&dump[lane][0];
    const unsigned ainc = qlast ? 64u : 0u;
    asm volatile(
#include "ga_biquad_pipe_asm.inc"
        : [w1] "+v"(w1), [w2] "+v"(w2), [w3] "+v"(w3), [y0] "+v"(yh[0]), [y1] "+v"(yh[1]), [y2] "+v"(yh[2]), [y3] "+v"(yh[3]), [nb] "+s"(nb)
        : [ab1] "v"(ab1), [ab2] "v"(ab2), [b0] "v"(b0), [ain] "v"(ain), [aout] "v"(aout), [ainc] "v"(ainc), [q0] "s"(q0mask)
        :
#include "ga_biquad_pipe_asm_clobbers.inc"
    );
  };
  // 16 steps of the fill / the drain of the pipeline, or past the end of a shorter cascade: lanes without a sample hold still
  auto masked = [&](int k0, int p0) {
#pragma unroll 4
    for (int i = 0; i < 16; i++) {
      const int j = k0 + i - jofs;
      const bool active = have && j >= 0 && j < n;
      const float up = dpp_left(yh[SK - 1]);
      const float x = q0 ? tile[srow][p0 + i] : up;
      const float w = x - ab1.x * w1 - ab2.x * w2;           // BiQuadFilterNode.cs:137
      const float yy = b0 * w + ab1.y * w1 + ab2.y * w2;     // :138
      w3 = active ? w2 : w3;
      w2 = active ? w1 : w2;
      w1 = active ? w : w1;
#pragma unroll
      for (int h = SK - 1; h > 0; h--) yh[h] = yh[h - 1];
      yh[0] = yy;
      if (qlast && active) tile[srow][p0 + i] = yy;
    }
  };
  const int nsteps = nmax + D;
  // (the coefficient and state loads complete HERE: left pending, their first use inside the loop would wait for vmcnt(0), that is
  // for the next tile's prefetch as well, once per tile -- the whole memory latency on the recurrence's clock)
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
  // Order of the memory operations of a tile: the samples of tile i + 1 are requested before tile i is walked and waited for
  // after it; the results of tile i leave AFTER that wait -- issued before it, every tile would wait for its stores to be
  // acknowledged (vmcnt counts loads and stores in one queue), a few microseconds on the recurrence's clock.
  v4f outv[MAXJ];
  bool out_whole = false;
  auto store_tile = [&](int base) {   // position p of the tile holds sample base + p - D
    if (out_whole) {
#pragma unroll
      for (int r = 0; r < MAXJ; r++)
        if (r < jcount) stg4((float*)bcast_ptr(outb, lane_of(r)) + (base - D) + 4 * lane, outv[r]);
      return;
    }
#pragma unroll
    for (int r = 0; r < MAXJ; r++) {
      if (r < jcount) {
        float* o = (float*)bcast_ptr(outb, lane_of(r));
        const int nr = __builtin_amdgcn_readlane(n, lane_of(r));
#pragma unroll
        for (int u = 0; u < TM; u++) {
          const int fi = base + 64 * u + lane - D;
          if (fi >= 0 && fi < nr) stg1(o + fi, outv[r][u]);
        }
      }
    }
  };
#ifdef GA_BQ_PROBE
  unsigned long long probe_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
  GA_BQ_T(tk0);
  fetch(0);
  for (int base = 0; base < nsteps; base += PT) {
    GA_BQ_T(ta);
    // (one explicit wait for the prefetch on every path: the compiler cannot see that a row without a cascade was never requested
    // and would otherwise wait for "its" load -- that is for the stores below -- when fetch() next overwrites the registers)
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
    if (pre_whole) {
#pragma unroll
      for (int r = 0; r < MAXJ; r++)
        if (r < jcount) *(v4f*)&tile[r][4 * lane] = pre[r];
    } else {
#pragma unroll
      for (int r = 0; r < MAXJ; r++)
        if (r < jcount) {
#pragma unroll
          for (int u = 0; u < TM; u++) tile[r][64 * u + lane] = pre[r][u];
        }
    }
    if (base > 0) store_tile(base - PT);
    __syncthreads();
    if (base + PT < nmax) fetch(base + PT);   // next tile's loads fly during the recurrence below
    GA_BQ_T(tb);
    // the tile's batches: [0, ps) masked (fill) | [ps, pe) steady, one assembly run | [pe, end) masked (drain, shorter cascades)
    const int pend = min(PT, (nsteps - base + 15) & ~15);
    const int ps = min(pend, max(0, (D - base + 15) & ~15));
    const int pe = max(ps, min(pend, (nmin - base) & ~15));
#pragma unroll 1
    for (int p0 = 0; p0 < ps; p0 += 16) { masked(base + p0, p0); GA_BQ_ACC(5, 1); }
    if (pe > ps) { steady_run(ps, (pe - ps) >> 4); GA_BQ_ACC(4, (pe - ps) >> 4); }
#pragma unroll 1
    for (int p0 = pe; p0 < pend; p0 += 16) { masked(base + p0, p0); GA_BQ_ACC(5, 1); }
    GA_BQ_T(tc);
    __syncthreads();
    out_whole = base >= D && base + PT - D <= nmin;
    if (out_whole) {
#pragma unroll
      for (int r = 0; r < MAXJ; r++)
        if (r < jcount) outv[r] = *(const v4f*)&tile[r][4 * lane];
    } else {
#pragma unroll
      for (int r = 0; r < MAXJ; r++)
        if (r < jcount) {
#pragma unroll
          for (int u = 0; u < TM; u++) outv[r][u] = tile[r][64 * u + lane];
        }
    }
    __syncthreads();
    GA_BQ_T(td);
    GA_BQ_ACC(0, tb - ta);
    GA_BQ_ACC(1, tc - tb);
    GA_BQ_ACC(2, td - tc);
  }
  store_tile((nsteps - 1) / PT * PT);
#ifdef GA_BQ_PROBE
  {
    GA_BQ_T(tk1);
    probe_acc[3] = tk1 - tk0;
    probe_acc[6] = 1;   // waves
    probe_acc[7] = (unsigned long long)jcount;
    if (lane == 0)
      for (int i = 0; i < 8; i++) atomicAdd(&ga_bq_probe[i], probe_acc[i]);
  }
#endif
  if (have) {
    for (int t = 0; t < me.twins; t++) {   // (twin channels: BiquadJob::twins)
      stg1(st + 2 * t, w1);
      stg1(st + 2 * t + 1, w2);
    }
  }
}
template <int NSEC>
static void launch_biquad_pipe(hipStream_t s, const BiquadJob* jobs_dev, int njobs, const BiquadSection* secs_dev) {
  constexpr int MAXJ = 4 * (16 / NSEC) < 16 ? 4 * (16 / NSEC) : 16;
  // The walk is bound by one wave's instruction issue, not by lanes, and a cascade more in a wave costs ~200 cycles of staging per
  // tile of 256 steps (12,200): up to 512 waves (one per two SIMDs) one cascade each, then fuller waves -- measured on MI355X
  // (tools/micro/bq_pipe_probe.hip, 4096 cascades of 5 sections x 120,000 frames): 512 waves of 8: 3.1-3.2 ms, 342 of 12: 3.1-3.3.
  int jpw = std::min(MAXJ, std::max(1, (njobs + 511) / 512));
  if (const char* e = expenv("GA_BQ_JPW")) jpw = std::min(MAXJ, std::max(1, atoi(e)));
  hipLaunchKernelGGL(biquad_pipe_kernel<NSEC>, dim3((njobs + jpw - 1) / jpw), dim3(64), 0, s, jobs_dev, njobs, secs_dev, jpw);
}
// ---- ONE section per job, one job per lane, nothing staged --------------------------------------------------------------------
// The pieces of cascades that are split along time (BiquadScanJob: tens of thousands of short walks) and any other single
// section.  The lane-per-cascade kernel above stages [jobs][frames] tiles through LDS so that every global access is a coalesced
// row -- ~80 instructions per row and tile of 64 frames, 85 per step of a 64-lane wave, and a wave pays ~5 cycles per instruction
// (config 2: 0.41 ms per pass over 0.49 GB).  Here a lane reads ITS piece 16 bytes at a time (four consecutive loads of a lane
// cover one 64-byte line, which the vector cache keeps), walks the four samples in registers -- the two packed products of w[n-1]
// ({a1, b1} w, {a2, b2} w) serve the recursion and the output half alike, 7 instructions per sample, 3 when only the state is
// wanted -- and writes 16 bytes.  The arithmetic is BiQuadFilterNode.cs:137-138 operation by operation (as biquad_pipe_kernel).
template <bool STATE_ONLY>
__global__ __launch_bounds__(64) void biquad1_kernel(const BiquadJob* __restrict jobs, int njobs, const BiquadSection* __restrict secs) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= njobs) return;
  const BiquadJob me = jobs[j];
  const BiquadSection sc = secs[me.sec0];
  float* st = me.state ? me.state : sc.state;
  const float b0 = sc.b0;
  const v2f ab1 = {sc.a1, sc.b1}, ab2 = {sc.a2, sc.b2};
  float w1 = ldg1(st), w2 = ldg1(st + 1);
  const float* __restrict in = me.in + me.f0;
  float* __restrict out = (!STATE_ONLY && me.out) ? me.out + me.f0 : nullptr;
  const int n = (int)me.n;
  v2f Bp = {ab2.x * w2, ab2.y * w2};   // {a2, b2} w[n-2]
  auto step = [&](float x) {
    const v2f A = {ab1.x * w1, ab1.y * w1};   // {a1, b1} w[n-1]
    const float t = x - A.x;
    const float w = t - Bp.x;                 // w = (x - a1 w1) - a2 w2
    float y = 0.f;
    if (!STATE_ONLY) {
      const float m = b0 * w;
      const float sum = m + A.y;
      y = sum + Bp.y;                         // y = (b0 w + b1 w1) + b2 w2
    }
    Bp = v2f{ab2.x * w1, ab2.y * w1};
    w2 = w1;
    w1 = w;
    return y;
  };
  // 32 frames = 128 bytes = one cache line of the lane's stream per round: the eight loads of a round go out back to back (the line is
  // used up while it is resident -- with 16 bytes per round the 64 lines of every wave of a CU evict each other between two uses and each
  // is fetched from L2 several times), the next round's are in flight during this round's 32 steps
  int i = 0;
  if (n >= 32) {
    v4f cur[8], nxt[8];
#pragma unroll
    for (int u = 0; u < 8; u++) cur[u] = ldg4(in + 4 * u);
    for (; i + 32 <= n; i += 32) {
      const bool more = i + 64 <= n;
#pragma unroll
      for (int u = 0; u < 8; u++) nxt[u] = more ? ldg4(in + i + 32 + 4 * u) : cur[u];
      v4f y[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        y[u].x = step(cur[u].x);
        y[u].y = step(cur[u].y);
        y[u].z = step(cur[u].z);
        y[u].w = step(cur[u].w);
      }
      if (!STATE_ONLY && out) {
#pragma unroll
        for (int u = 0; u < 8; u++) stg4(out + i + 4 * u, y[u]);
      }
#pragma unroll
      for (int u = 0; u < 8; u++) cur[u] = nxt[u];
    }
  }
  for (; i + 4 <= n; i += 4) {
    const v4f c = ldg4(in + i);
    const float y0 = step(c.x), y1 = step(c.y), y2 = step(c.z), y3 = step(c.w);
    if (!STATE_ONLY && out) stg4(out + i, v4f{y0, y1, y2, y3});
  }
  for (; i < n; i++) {
    const float y = step(ldg1(in + i));
    if (!STATE_ONLY && out) stg1(out + i, y);
  }
  for (int t = 0; t < me.twins; t++) {   // (twin channels: BiquadJob::twins)
    stg1(st + 2 * t, w1);
    stg1(st + 2 * t + 1, w2);
  }
}
void launch_biquad_lanes(hipStream_t s, const BiquadJob* jobs_dev, int njobs, const BiquadSection* secs_dev, int nsec, bool state_only) {
  if (njobs <= 0) return;
  static const bool staged1 = expenv("GA_BQ_STAGED1") != nullptr;   // (measurement: the staged kernel for single sections too)
  if (nsec == 1 && !staged1) {
    if (state_only)
      hipLaunchKernelGGL(biquad1_kernel<true>, dim3((njobs + 63) / 64), dim3(64), 0, s, jobs_dev, njobs, secs_dev);
    else
      hipLaunchKernelGGL(biquad1_kernel<false>, dim3((njobs + 63) / 64), dim3(64), 0, s, jobs_dev, njobs, secs_dev);
    return;
  }
  if (njobs <= 16 * 1024) launch_biquad_jpw<32>(s, jobs_dev, njobs, secs_dev, nsec);   // (more, emptier waves while the chip has room)
  else launch_biquad_jpw<64>(s, jobs_dev, njobs, secs_dev, nsec);
}
// the pieces of every cascade as jobs of the lane-per-cascade kernel: thread = (cascade, piece)
__global__ __launch_bounds__(256) void biquad_split_expand_kernel(const BiquadScanJob* __restrict casc, int ncasc, int G, int64_t K,
                                                                 BiquadJob* __restrict passA, BiquadJob* __restrict passB) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= ncasc * G) return;
  const int j = v / G, l = v % G;
  const BiquadScanJob C = casc[j];
  BiquadJob b;
  b.in = C.in;
  b.out = C.out;
  b.sec0 = C.sec0;
  b.nsec = C.nsec;
  b.f0 = C.f0 + (int64_t)l * K;
  b.n = min(K, C.n - (int64_t)l * K);
  b.state = l + 1 < G ? C.scratch + (size_t)l * C.nsec * 2 : nullptr;   // the last piece runs on the cascade's own state
  b.twins = l + 1 < G ? 1 : C.twins;
  b.pad_ = 0;
  passB[(size_t)j * G + l] = b;
  if (l + 1 < G) {
    b.out = nullptr;
    b.twins = 1;
    passA[(size_t)j * (G - 1) + l] = b;
  }
}
void launch_biquad_split_expand(hipStream_t s, const BiquadScanJob* casc_dev, int ncasc, int G, int64_t K, BiquadJob* passA, BiquadJob* passB) {
  if (ncasc <= 0) return;
  hipLaunchKernelGGL(biquad_split_expand_kernel, dim3((ncasc * G + 255) / 256), dim3(256), 0, s, casc_dev, ncasc, G, K, passA, passB);
}
// s_{l+1} = A^K s_l + z_l (float64 accumulation); one thread per cascade
__global__ __launch_bounds__(64) void biquad_scan_kernel(const BiquadScanJob* __restrict jobs, int njobs, int G, const BiquadSection* __restrict secs,
                                                        const uint8_t* __restrict tables) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= njobs) return;
  const BiquadScanJob J = jobs[j];
  const int D = 2 * J.nsec;
  const GA_GLOBAL double* Mg = (const GA_GLOBAL double*)(tables + J.m_off);
  double cur[2 * kMaxBiquadSections], nxt[2 * kMaxBiquadSections];
  for (int q = 0; q < J.nsec; q++) {
    const float* st = secs[J.sec0 + q].state;
    cur[2 * q] = ldg1(st);
    cur[2 * q + 1] = ldg1(st + 1);
  }
  for (int l = 0; l + 1 < G; l++) {
    float* sc = J.scratch + (size_t)l * D;
    for (int r = 0; r < D; r++) {
      double a = (double)ldg1(sc + r);   // z_l
      for (int c = 0; c < D; c++) a += Mg[r * D + c] * cur[c];
      nxt[r] = a;
    }
    for (int r = 0; r < D; r++) {
      stg1(sc + r, (float)cur[r]);       // s_l: where pass B's piece l starts
      cur[r] = (double)(float)nxt[r];    // (the state is float in the filter)
    }
  }
  for (int q = 0; q < J.nsec; q++) {     // s_{G-1}: the last piece starts from (and ends in) the cascade's own state
    float* st = secs[J.sec0 + q].state;
    stg1(st, (float)cur[2 * q]);
    stg1(st + 1, (float)cur[2 * q + 1]);
  }
}
// The same scan with the cascade length known at compile time: state, matrix and the pieces' z_l live in registers (with a run-time
// length they are indexed arrays in scratch memory, and every step waits for its own loads: 0.19 ms for config 2's 255 steps), and
// z_{l+1} is requested before s_l is written over z_l.  Same operations in the same order: the same bits.
template <int NS>
__global__ __launch_bounds__(64) void biquad_scan_fixed_kernel(const BiquadScanJob* __restrict jobs, int njobs, int G, const BiquadSection* __restrict secs,
                                                              const uint8_t* __restrict tables) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= njobs) return;
  const BiquadScanJob J = jobs[j];
  constexpr int D = 2 * NS;
  const GA_GLOBAL double* Mg = (const GA_GLOBAL double*)(tables + J.m_off);
  double M[D * D];
#pragma unroll
  for (int e = 0; e < D * D; e++) M[e] = Mg[e];
  double cur[D];
#pragma unroll
  for (int q = 0; q < NS; q++) {
    const float* st = secs[J.sec0 + q].state;
    cur[2 * q] = ldg1(st);
    cur[2 * q + 1] = ldg1(st + 1);
  }
  float zn[D];
  if (G > 1) {
#pragma unroll
    for (int r = 0; r < D; r++) zn[r] = ldg1(J.scratch + r);
  }
  // (the matrix and state loads complete HERE: left pending, their first use inside the loop waits for vmcnt(0), that is for the
  // prefetch of z_{l+1} issued just before it, in every step -- 28 instead of 20 us for config 2's 255 steps)
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
  for (int l = 0; l + 1 < G; l++) {
    float* sc = J.scratch + (size_t)l * D;
    float z[D];
#pragma unroll
    for (int r = 0; r < D; r++) z[r] = zn[r];
    if (l + 2 < G) {
#pragma unroll
      for (int r = 0; r < D; r++) zn[r] = ldg1(sc + D + r);
    }
    double nxt[D];
#pragma unroll
    for (int r = 0; r < D; r++) {
      double a = (double)z[r];   // z_l
#pragma unroll
      for (int c = 0; c < D; c++) a += M[r * D + c] * cur[c];
      nxt[r] = a;
    }
#pragma unroll
    for (int r = 0; r < D; r++) {
      stg1(sc + r, (float)cur[r]);       // s_l: where pass B's piece l starts
      cur[r] = (double)(float)nxt[r];    // (the state is float in the filter)
    }
  }
#pragma unroll
  for (int q = 0; q < NS; q++) {
    float* st = secs[J.sec0 + q].state;
    stg1(st, (float)cur[2 * q]);
    stg1(st + 1, (float)cur[2 * q + 1]);
  }
}
// (the launch's jobs all have `nsec` sections: Exec::bqScans is kept by cascade length)
void launch_biquad_scan(hipStream_t s, const BiquadScanJob* jobs_dev, int njobs, int G, const BiquadSection* secs_dev, const uint8_t* tables, int nsec) {
  if (njobs <= 0) return;
  const dim3 g((njobs + 63) / 64), b(64);
  switch (nsec) {
    case 1: hipLaunchKernelGGL(biquad_scan_fixed_kernel<1>, g, b, 0, s, jobs_dev, njobs, G, secs_dev, tables); return;
    case 2: hipLaunchKernelGGL(biquad_scan_fixed_kernel<2>, g, b, 0, s, jobs_dev, njobs, G, secs_dev, tables); return;
    case 3: hipLaunchKernelGGL(biquad_scan_fixed_kernel<3>, g, b, 0, s, jobs_dev, njobs, G, secs_dev, tables); return;
    case 4: hipLaunchKernelGGL(biquad_scan_fixed_kernel<4>, g, b, 0, s, jobs_dev, njobs, G, secs_dev, tables); return;
    default: break;
  }
  hipLaunchKernelGGL(biquad_scan_kernel, g, b, 0, s, jobs_dev, njobs, G, secs_dev, tables);
}
void launch_biquad(hipStream_t s, const BiquadJob* jobs_dev, int njobs, const BiquadSection* secs_dev, int nsec) {
  if (njobs <= 0) return;
  static const bool pipe = !expenv("GA_BQ_NOPIPE");
  if (pipe && nsec >= 2) {
    switch (nsec) {
      case 2: launch_biquad_pipe<2>(s, jobs_dev, njobs, secs_dev); return;
      case 3: launch_biquad_pipe<3>(s, jobs_dev, njobs, secs_dev); return;
      case 4: launch_biquad_pipe<4>(s, jobs_dev, njobs, secs_dev); return;
      case 5: launch_biquad_pipe<5>(s, jobs_dev, njobs, secs_dev); return;
      case 6: launch_biquad_pipe<6>(s, jobs_dev, njobs, secs_dev); return;
      case 7: launch_biquad_pipe<7>(s, jobs_dev, njobs, secs_dev); return;
      default: launch_biquad_pipe<8>(s, jobs_dev, njobs, secs_dev); return;
    }
  }
  // measured on MI355X (config 4, 8,192 cascades of 5 sections): ~512 waves on the chip (one per two SIMDs) is the sweet
  // spot -- 4 / 8 / 16 / 32 jobs per wave took 81 / 65 / 47 / 54 ms.  A wave issues one VALU instruction per ~4 cycles
  // however many lanes are busy, so fewer, fuller waves only pay once that many waves exist.
  int per = (njobs + 511) / 512;
  if (const char* e = expenv("GA_BQ_JPW")) per = atoi(e);   // tuning override
  if (per <= 4) launch_biquad_jpw<4>(s, jobs_dev, njobs, secs_dev, nsec);
  else if (per <= 8) launch_biquad_jpw<8>(s, jobs_dev, njobs, secs_dev, nsec);
  else if (per <= 16) launch_biquad_jpw<16>(s, jobs_dev, njobs, secs_dev, nsec);
  else if (per <= 32) launch_biquad_jpw<32>(s, jobs_dev, njobs, secs_dev, nsec);
  else launch_biquad_jpw<64>(s, jobs_dev, njobs, secs_dev, nsec);
}

// ---- BiQuadFilterNode with automated parameters --------------------------------------------------------
// LX (option "libm_exact"): cosf / sinf / powf as glibc computes them (ga_libmf.hpp) in place of the double-precision functions rounded once
template <bool LX>
__device__ void biquad_update_coefficients(int type, float frequency, float q, float gain, float sample_rate, float& b0, float& b1,
                                           float& b2, float& a1, float& a2) {   // BiQuadFilterNode.cs:149-258
  const float PI = 3.14159274f;
  float w0 = 2.f * PI * frequency / sample_rate;
  // The reference's MathF.Cos / MathF.Sin are the C library's, which evaluate in double and round once; the device library's
  // single-precision versions are 1-2 ulp off that, which a resonant section amplifies ~fs/(pi*f/Q) times.  Evaluating in
  // double here lands on the same float except when the true value sits within ~1e-9 of a rounding boundary.
  float cosW0 = LX ? ga_cosf(w0) : (float)cos((double)w0);
  float sinW0 = LX ? ga_sinf(w0) : (float)sin((double)w0);
  float alpha = sinW0 / (2.f * q);
  float a0, A1, A2, B0, B1, B2;
  switch (type) {
    case 0: B0 = (1.f - cosW0) / 2.f; B1 = 1.f - cosW0; B2 = (1.f - cosW0) / 2.f; a0 = 1.f + alpha; A1 = -2.f * cosW0; A2 = 1.f - alpha; break;
    case 1: B0 = (1.f + cosW0) / 2.f; B1 = -(1.f + cosW0); B2 = (1.f + cosW0) / 2.f; a0 = 1.f + alpha; A1 = -2.f * cosW0; A2 = 1.f - alpha; break;
    case 2: B0 = alpha; B1 = 0.f; B2 = -alpha; a0 = 1.f + alpha; A1 = -2.f * cosW0; A2 = 1.f - alpha; break;
    case 3: B0 = 1.f; B1 = -2.f * cosW0; B2 = 1.f; a0 = 1.f + alpha; A1 = -2.f * cosW0; A2 = 1.f - alpha; break;
    case 4: B0 = 1.f - alpha; B1 = -2.f * cosW0; B2 = 1.f + alpha; a0 = 1.f + alpha; A1 = -2.f * cosW0; A2 = 1.f - alpha; break;
    case 5: {
      float A = LX ? ga_powf(10.f, gain / 40.f) : (float)pow(10.0, (double)(gain / 40.f));
      B0 = 1.f + alpha * A; B1 = -2.f * cosW0; B2 = 1.f - alpha * A; a0 = 1.f + alpha / A; A1 = -2.f * cosW0; A2 = 1.f - alpha / A;
      break;
    }
    case 6: {
      float A = LX ? ga_powf(10.f, gain / 40.f) : (float)pow(10.0, (double)(gain / 40.f));
      float beta = sqrtf(A) / q;
      B0 = A * ((A + 1.f) - (A - 1.f) * cosW0 + beta * sinW0);
      B1 = 2.f * A * ((A - 1.f) - (A + 1.f) * cosW0);
      B2 = A * ((A + 1.f) - (A - 1.f) * cosW0 - beta * sinW0);
      a0 = (A + 1.f) + (A - 1.f) * cosW0 + beta * sinW0;
      A1 = -2.f * ((A - 1.f) + (A + 1.f) * cosW0);
      A2 = (A + 1.f) + (A - 1.f) * cosW0 - beta * sinW0;
      break;
    }
    case 7: {
      float A = LX ? ga_powf(10.f, gain / 40.f) : (float)pow(10.0, (double)(gain / 40.f));
      float beta = sqrtf(A) / q;
      B0 = A * ((A + 1.f) + (A - 1.f) * cosW0 + beta * sinW0);
      B1 = -2.f * A * ((A - 1.f) + (A + 1.f) * cosW0);
      B2 = A * ((A + 1.f) + (A - 1.f) * cosW0 - beta * sinW0);
      a0 = (A + 1.f) - (A - 1.f) * cosW0 + beta * sinW0;
      A1 = 2.f * ((A - 1.f) - (A + 1.f) * cosW0);
      A2 = (A + 1.f) - (A - 1.f) * cosW0 - beta * sinW0;
      break;
    }
    default: B0 = 1.f; B1 = 0.f; B2 = 0.f; a0 = 1.f; A1 = 0.f; A2 = 0.f; break;
  }
  b0 = B0 / a0;
  b1 = B1 / a0;
  b2 = B2 / a0;
  a1 = A1 / a0;
  a2 = A2 / a0;
}
template <bool LX>
__global__ __launch_bounds__(64) void biquad_dynamic_kernel(const BiquadDynJob* __restrict jobs, int njobs) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= njobs) return;
  const BiquadDynJob* __restrict job = &jobs[j];
  GA_GLOBAL BiquadDynState* st = gptr(job->state);
  float b0 = st->b0, b1 = st->b1, b2 = st->b2, a1 = st->a1, a2 = st->a2;
  // (bit 8 of filter_type: the Type setter ran on the host while the state lived here -- _coefficientsDirty, BiQuadFilterNode.cs:24-36)
  bool dirty = st->dirty != 0 || (job->filter_type & 0x100) != 0;
  const int C = job->channels;
  const int type = job->filter_type & 0xFF;
  const float nyq = job->nyquist, sr = job->sample_rate;
  for (int64_t b = 0; b < job->nblocks; b++) {
    const int64_t f0 = (job->b0 + b) * kBlock;
    const float gainDb = job->gcurve ? ldg1(job->gcurve + f0) : job->gval;
    float lb0 = b0, lb1 = b1, lb2 = b2, la1 = a1, la2 = a2;   // lastB0 ... (:110)
    float usedFreq = 1000.f, usedQ = 1.0f;                     // _lastFrequency / _lastQ never change (:13-14,111-112)
    for (int ch = 0; ch < C; ch++) {
      const GA_GLOBAL float* in = gptr(job->in[ch]);
      GA_GLOBAL float* out = gptr(job->out[ch]);
      float w1 = st->w[2 * ch], w2 = st->w[2 * ch + 1];
      for (int i = 0; i < kBlock; i++) {
        float f = job->fcurve ? ldg1(job->fcurve + f0 + i) : job->fval;
        f = f < 1.f ? 1.f : (f > nyq ? nyq : f);
        float q = job->qcurve ? ldg1(job->qcurve + f0 + i) : job->qval;
        q = max_ref(0.001f, q);   // Math.Max (:124): a NaN Q stays NaN -- no update unless the frequency moves, then NaN coefficients
        if (dirty || fabsf(f - usedFreq) > 0.001f || fabsf(q - usedQ) > 0.0001f) {   // usedGain == gainDb always (:113,126)
          biquad_update_coefficients<LX>(type, f, q, gainDb, sr, b0, b1, b2, a1, a2);
          usedFreq = f;
          usedQ = q;
          dirty = false;
          lb0 = b0; lb1 = b1; lb2 = b2; la1 = a1; la2 = a2;
        }
        float x = in ? in[f0 + i] : 0.f;
        float w = x - la1 * w1 - la2 * w2;
        float y = lb0 * w + lb1 * w1 + lb2 * w2;
        w2 = w1;
        w1 = w;
        out[f0 + i] = y;
      }
      st->w[2 * ch] = w1;
      st->w[2 * ch + 1] = w2;
    }
  }
  st->b0 = b0; st->b1 = b1; st->b2 = b2; st->a1 = a1; st->a2 = a2;
  st->dirty = dirty ? 1 : 0;
}
void launch_biquad_dynamic(hipStream_t s, const BiquadDynJob* jobs_dev, int njobs, bool libm_exact) {
  if (njobs <= 0) return;
  if (libm_exact) hipLaunchKernelGGL(biquad_dynamic_kernel<true>, dim3((njobs + 63) / 64), dim3(64), 0, s, jobs_dev, njobs);
  else hipLaunchKernelGGL(biquad_dynamic_kernel<false>, dim3((njobs + 63) / 64), dim3(64), 0, s, jobs_dev, njobs);
}

}  // namespace ga
