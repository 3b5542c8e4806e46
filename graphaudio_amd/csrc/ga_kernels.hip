// ga_kernels.hip -- the element-wise node kernels of the GraphAudio offline render path, hand-written for gfx950 (CDNA4,
// MI355X): mix / downmix / gain, the AudioParam timeline and modulation, the buffer, stream and constant sources with their
// resamplers, the oscillator, both stereo panners, the delay kernels and the output interleave.  They restate AudioNodeInput.cs,
// GainNode.cs, AudioParam.cs, AudioBufferSourceNode.cs, CubicResampler.cs, AudioStreamNodeBase, ConstantSourceNode,
// OscillatorNode.cs, StereoPannerNode and DelayNode of the-byte-bender/GraphAudio; each kernel cites what it reproduces as
// (file:line).  The other kernel families have a file each: ga_rfft.hip (256-point real FFT), ga_conv.hip (fine-partition
// convolver), ga_coarse.hip (coarse-partition convolver), ga_biquad.hip (BiQuadFilterNode), ga_spatial.hip (SpatialPannerNode).
//
// Notes that hold for every kernel file (DESIGN.md has the full account):
//  * wavefront = 64 lanes everywhere.
//  * serial-in-time recurrences (biquad, resampler) stage 64x64 tiles through LDS so HBM accesses stay coalesced.
//  * compiled with -ffp-contract=off: float32 elementwise arithmetic is unfused like the reference's; fused multiply-adds
//    appear only where written explicitly (fma(), MFMA).

#include "ga_kernels.hpp"
#include "ga_device_common.hpp"
#include "ga_gsr.hpp"
#include "ga_fft16.hpp"
#include "ga_libmf.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

namespace ga {

// =====================================================================================================
//  Mix (AudioNodeInput.Pull / MixBuffer, AudioNodeInput.cs:100-244): sequential float32 sum in connection order,
//  starting from the cleared buffer (0 + t0 + t1 + ...), one thread per 1 or 4 frames.
// =====================================================================================================
template <int VEC, bool SCALED>
__global__ __launch_bounds__(256) void mix_kernel(const MixJob* __restrict jobs, const float* const* __restrict terms, const float* __restrict gains,
                                                  const float* const* __restrict curves) {
  const MixJob job = jobs[blockIdx.y];
  const int64_t nv = (job.n + VEC - 1) / VEC;
  const float* const* __restrict tp = terms + job.term0;
  const float* __restrict gp = SCALED ? gains + job.term0 : nullptr;   // SCALED: term j contributes fl(x * gain[j]) -- a folded constant GainNode
  // ... or fl(x * curve_j[f]) where the folded GainNode's gain follows a timeline (curves[j] != null): GainNode.cs:52-57
  const float* const* __restrict cp = (SCALED && curves) ? curves + job.term0 : nullptr;
  if (SCALED && job.nterms == 1) {   // a gain on its own: out = in * g, as gain_kernel writes it (no 0 + in front)
    const float g = gp[0];
    const float* __restrict cv = cp ? cp[0] : nullptr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
      const int64_t f = job.f0 + i * VEC;
      if (VEC == 4) {
        const v4f v = ldg4(tp[0] + f);
        const v4f gv = cv ? ldg4(cv + f) : v4f{g, g, g, g};
        const v4f r = v4f{v.x * gv.x, v.y * gv.y, v.z * gv.z, v.w * gv.w};
        stg4(job.out + f, r);
        if (job.out2) stg4(job.out2 + f, r);
      } else {
        const float r = ldg1(tp[0] + f) * (cv ? ldg1(cv + f) : g);
        gptr(job.out)[f] = r;
        if (job.out2) gptr(job.out2)[f] = r;
      }
    }
    return;
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = job.f0 + i * VEC;
    if (VEC == 4) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      int j = 0;
      for (; j + 4 <= job.nterms; j += 4) {   // four loads in flight, adds strictly in term order
        v4f v0 = ldg4(tp[j] + f);
        v4f v1 = ldg4(tp[j + 1] + f);
        v4f v2 = ldg4(tp[j + 2] + f);
        v4f v3 = ldg4(tp[j + 3] + f);
        if (SCALED) {   // (products rounded on their own: -ffp-contract=off, no fma with the add below)
          const float g0 = gp[j], g1 = gp[j + 1], g2 = gp[j + 2], g3 = gp[j + 3];
          v4f m0 = v4f{g0, g0, g0, g0}, m1 = v4f{g1, g1, g1, g1}, m2 = v4f{g2, g2, g2, g2}, m3 = v4f{g3, g3, g3, g3};
          if (cp) {
            if (cp[j]) m0 = ldg4(cp[j] + f);
            if (cp[j + 1]) m1 = ldg4(cp[j + 1] + f);
            if (cp[j + 2]) m2 = ldg4(cp[j + 2] + f);
            if (cp[j + 3]) m3 = ldg4(cp[j + 3] + f);
          }
          v0 = v4f{v0.x * m0.x, v0.y * m0.y, v0.z * m0.z, v0.w * m0.w};
          v1 = v4f{v1.x * m1.x, v1.y * m1.y, v1.z * m1.z, v1.w * m1.w};
          v2 = v4f{v2.x * m2.x, v2.y * m2.y, v2.z * m2.z, v2.w * m2.w};
          v3 = v4f{v3.x * m3.x, v3.y * m3.y, v3.z * m3.z, v3.w * m3.w};
        }
        acc.x += v0.x; acc.y += v0.y; acc.z += v0.z; acc.w += v0.w;
        acc.x += v1.x; acc.y += v1.y; acc.z += v1.z; acc.w += v1.w;
        acc.x += v2.x; acc.y += v2.y; acc.z += v2.z; acc.w += v2.w;
        acc.x += v3.x; acc.y += v3.y; acc.z += v3.z; acc.w += v3.w;
      }
      for (; j < job.nterms; j++) {
        v4f v = ldg4(tp[j] + f);
        if (SCALED) {
          const float g = gp[j];
          const v4f m = (cp && cp[j]) ? ldg4(cp[j] + f) : v4f{g, g, g, g};
          v = v4f{v.x * m.x, v.y * m.y, v.z * m.z, v.w * m.w};
        }
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
      }
      stg4(job.out + f, v4f{acc.x, acc.y, acc.z, acc.w});
      if (job.out2) stg4(job.out2 + f, v4f{acc.x, acc.y, acc.z, acc.w});
    } else {
      float acc = 0.f;
      for (int j = 0; j < job.nterms; j++) {
        float v = ldg1(tp[j] + f);
        if (SCALED) v = v * ((cp && cp[j]) ? ldg1(cp[j] + f) : gp[j]);
        acc += v;
      }
      gptr(job.out)[f] = acc;
      if (job.out2) gptr(job.out2)[f] = acc;
    }
  }
}
void launch_mix(hipStream_t s, const MixJob* jobs_dev, int njobs, const float* const* terms_dev, int64_t max_n, bool vec4, const float* gains_dev,
                const float* const* curves_dev) {
  if (njobs <= 0 || max_n <= 0) return;
  int64_t nv = vec4 ? (max_n + 3) / 4 : max_n;
  int gx = (int)std::min<int64_t>((nv + 255) / 256, 2048);
  if (gains_dev) {
    if (vec4)
      GA_LAUNCH_JOBS((mix_kernel<4, true>), gx, 256, jobs_dev, njobs, terms_dev, gains_dev, curves_dev);
    else
      GA_LAUNCH_JOBS((mix_kernel<1, true>), gx, 256, jobs_dev, njobs, terms_dev, gains_dev, curves_dev);
  } else if (vec4) {
    GA_LAUNCH_JOBS((mix_kernel<4, false>), gx, 256, jobs_dev, njobs, terms_dev, gains_dev, curves_dev);
  } else {
    GA_LAUNCH_JOBS((mix_kernel<1, false>), gx, 256, jobs_dev, njobs, terms_dev, gains_dev, curves_dev);
  }
}

// ---- a bus of MANY terms (hundreds to thousands of voices into one input): few jobs, each a long strictly ordered sum ----------
// With one job per channel the launch above is a few hundred waves whose every step waits for a scalar load (the term's pointer,
// gain, curve) and then for a vector load: at 4 terms per step a 4096-term bus is 1024 such round trips per wave (measured: 0.95 ms
// for 2 x 4096 terms x 120,000 frames, 0.26 of the HBM rate).  Here a wave takes 64 frames, one per lane, reads the descriptors of
// 64 terms with ONE coalesced load each (pointer / gain / curve: lane l holds term t0 + l, handed out with v_readlane) and keeps
// the loads of 32 terms in flight; the additions stay in term order (AudioNodeInput.cs:118-132).
template <bool SCALED>
__global__ __launch_bounds__(64) void mix_wide_kernel(const MixJob* __restrict jobs, const float* const* __restrict terms, const float* __restrict gains,
                                                     const float* const* __restrict curves) {
  const MixJob job = jobs[blockIdx.y];
  const int lane = threadIdx.x;
  const float* const* __restrict tp = terms + job.term0;
  const float* __restrict gp = SCALED ? gains + job.term0 : nullptr;
  const float* const* __restrict cp = (SCALED && curves) ? curves + job.term0 : nullptr;
  constexpr int NB = 32;
  for (int64_t i0 = (int64_t)blockIdx.x * 64; i0 < job.n; i0 += (int64_t)gridDim.x * 64) {
    const int64_t i = i0 + lane;
    const bool live = i < job.n;
    const int64_t f = job.f0 + (live ? i : 0);
    float acc = 0.f;
    for (int t0 = 0; t0 < job.nterms; t0 += 64) {
      const int cnt = min(64, job.nterms - t0);
      const bool mine = lane < cnt;
      const float* myp = mine ? tp[t0 + lane] : nullptr;
      const float myg = (SCALED && mine) ? gp[t0 + lane] : 1.f;
      const float* myc = (cp && mine) ? cp[t0 + lane] : nullptr;
      auto ptr_of = [](const float* p, int l) {
        const unsigned long long v = (unsigned long long)p;
        const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, l), hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), l);
        return (const float*)(((unsigned long long)hi << 32) | lo);
      };
#pragma unroll
      for (int u0 = 0; u0 < 64; u0 += NB) {
        if (u0 >= cnt) break;
        if (u0 + NB <= cnt) {
          float v[NB], m[NB];
#pragma unroll
          for (int u = 0; u < NB; u++) v[u] = ldg1(ptr_of(myp, u0 + u) + f);
          if (SCALED) {
#pragma unroll
            for (int u = 0; u < NB; u++) {
              m[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(myg), u0 + u));
              if (cp) {
                const float* c = ptr_of(myc, u0 + u);
                if (c) m[u] = ldg1(c + f);
              }
            }
#pragma unroll
            for (int u = 0; u < NB; u++) v[u] = v[u] * m[u];   // (rounded on its own: -ffp-contract=off)
          }
#pragma unroll
          for (int u = 0; u < NB; u++) acc += v[u];
        } else {
          for (int u = u0; u < cnt; u++) {   // the last, partial batch of the bus
            float v = ldg1(tp[t0 + u] + f);
            if (SCALED) v = v * ((cp && cp[t0 + u]) ? ldg1(cp[t0 + u] + f) : gp[t0 + u]);
            acc += v;
          }
        }
      }
    }
    if (live) {
      gptr(job.out)[f] = acc;
      if (job.out2) gptr(job.out2)[f] = acc;
    }
  }
}
void launch_mix_wide(hipStream_t s, const MixJob* jobs_dev, int njobs, const float* const* terms_dev, int64_t max_n, const float* gains_dev,
                     const float* const* curves_dev) {
  if (njobs <= 0 || max_n <= 0) return;
  const int gx = (int)std::min<int64_t>((max_n + 63) / 64, 8192);
  if (gains_dev)
    GA_LAUNCH_JOBS((mix_wide_kernel<true>), gx, 64, jobs_dev, njobs, terms_dev, gains_dev, curves_dev);
  else
    GA_LAUNCH_JOBS((mix_wide_kernel<false>), gx, 64, jobs_dev, njobs, terms_dev, gains_dev, curves_dev);
}

template <bool SCALED>
__global__ __launch_bounds__(256) void downmix_kernel(const DownmixJob* __restrict jobs, const float* const* __restrict terms, const float* __restrict gains) {
  const DownmixJob job = jobs[blockIdx.y];
  const float* const* __restrict tp = terms + job.term0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < job.n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = job.f0 + i;
    float sum = 0.f;
    for (int ch = 0; ch < job.nch; ch++) {   // AudioNodeInput.cs:221-226
      float v = ldg1(tp[ch] + f);
      if (SCALED) v = v * gains[job.term0 + ch];
      sum += v;
    }
    gptr(job.out)[f] = sum * job.scale;
  }
}
void launch_downmix(hipStream_t s, const DownmixJob* jobs_dev, int njobs, const float* const* terms_dev, int64_t max_n, const float* gains_dev) {
  if (njobs <= 0 || max_n <= 0) return;
  int gx = (int)std::min<int64_t>((max_n + 255) / 256, 2048);
  if (gains_dev) GA_LAUNCH_JOBS(downmix_kernel<true>, gx, 256, jobs_dev, njobs, terms_dev, gains_dev);
  else GA_LAUNCH_JOBS(downmix_kernel<false>, gx, 256, jobs_dev, njobs, terms_dev, gains_dev);
}

// ---- GainNode (GainNode.cs:48-58) ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void gain_kernel(const GainJob* __restrict jobs) {
  const GainJob job = jobs[blockIdx.y];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < job.n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = job.f0 + i;
    float g = job.curve ? gptr(job.curve)[f] : job.gain;
    if (job.mod) {   // Math.Clamp(intrinsicValue + modulation, min, max), AudioParam.cs:129
      g = clamp_ref(g + gptr(job.mod)[f], job.vmin, job.vmax);
    }
    gptr(job.out)[f] = gptr(job.in)[f] * g;
  }
}
void launch_gain(hipStream_t s, const GainJob* jobs_dev, int njobs, int64_t max_n) {
  if (njobs <= 0 || max_n <= 0) return;
  int gx = (int)std::min<int64_t>((max_n + 255) / 256, 1024);
  GA_LAUNCH_JOBS(gain_kernel, gx, 256, jobs_dev, njobs);
}

// =====================================================================================================
//  AudioParam timeline (AudioParam.ComputeValueAtTime and helpers, AudioParam.cs:169-247), double precision,
//  no contraction: sampleTime = blockTime + i * deltaTime (:116-120); k-rate samples at block start (:146).
// =====================================================================================================
__global__ __launch_bounds__(128) void param_curve_kernel(const ParamJob* __restrict jobs, const ParamEvent* __restrict events,
                                                          const double* __restrict block_times, double delta_time) {
  const ParamJob job = jobs[blockIdx.y];
  const int i = threadIdx.x;
  for (int64_t b = blockIdx.x; b < job.nblocks; b += gridDim.x) {
    const int64_t blk = job.b0 + b;
    const double bt = block_times[blk];
    double st = job.arate ? bt + i * delta_time : bt;
    gptr(job.out)[blk * kBlock + i] = param_value_at(events + job.ev0, job.nev, job.value, st);
  }
}
void launch_param_curve(hipStream_t s, const ParamJob* jobs_dev, int njobs, const ParamEvent* events_dev,
                        const double* block_times_dev, double delta_time, int64_t max_blocks) {
  if (njobs <= 0 || max_blocks <= 0) return;
  int gx = (int)std::min<int64_t>(max_blocks, 4096);
  GA_LAUNCH_JOBS(param_curve_kernel, gx, 128, jobs_dev, njobs, events_dev, block_times_dev, delta_time);
}

// ---- looping rate-1 source (AudioBufferSourceNode.cs:186-235) --------------------------------------------
__global__ __launch_bounds__(256) void loop_source_kernel(const LoopJob* __restrict jobs) {
  const LoopJob job = jobs[blockIdx.y];
  const int64_t len = job.loop_end - job.loop_start;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < job.n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t u = job.pos0 + i;
    if (u >= job.loop_end) u = job.loop_start + (len > 0 ? (u - job.loop_end) % len : 0);
    gptr(job.out)[job.f0 + i] = gptr(job.buf)[u];
  }
}
void launch_loop_source(hipStream_t s, const LoopJob* jobs_dev, int njobs, int64_t max_n) {
  if (njobs <= 0 || max_n <= 0) return;
  int gx = (int)std::min<int64_t>((max_n + 255) / 256, 1024);
  GA_LAUNCH_JOBS(loop_source_kernel, gx, 256, jobs_dev, njobs);
}

// =====================================================================================================
//  CubicResampler (CubicResampler.cs:26-63).  The double-precision position recurrence is replayed on the host
//  once per distinct rate (the "trajectory"); every (job, block) pair is then independent: one lane walks the 128
//  outputs of its block with exactly the reference's per-sample arithmetic.  64 consecutive blocks of one job per
//  wavefront; outputs go through LDS so the HBM stores are coalesced.
// =====================================================================================================
// CubicResampler.cs:52-57, the reference's expression tree (the build has -ffp-contract=off: the tree is the result)
__device__ __forceinline__ float cubic_interp(float S0, float S1, float S2, float S3, float t) {
  return S1 + t * (0.5f * (S2 - S0) + t * ((S0 - 2.5f * S1 + 2.f * S2 - 0.5f * S3) + t * (0.5f * (S3 - S0) + 1.5f * (S1 - S2))));
}
// the tile of a workgroup (one row per lane's block) -> `nb` consecutive blocks of `out`, coalesced
__device__ __forceinline__ void store_tile(const float (&tile)[64][kBlock + 1], GA_GLOBAL float* __restrict out, int nb, int lane) {
  for (int r = 0; r < nb; r++) {
    out[(int64_t)r * kBlock + lane] = tile[r][lane];
    out[(int64_t)r * kBlock + 64 + lane] = tile[r][64 + lane];
  }
}
__global__ __launch_bounds__(64) void resample_kernel(const ResampleJob* __restrict jobs, const ResampleBlock* __restrict traj) {
  __shared__ float tile[64][kBlock + 1];
  const ResampleJob job = jobs[blockIdx.y];
  const int lane = threadIdx.x;
  const int64_t bl0 = (int64_t)blockIdx.x * 64;
  if (bl0 >= job.nblocks) return;
  const int64_t b = bl0 + lane;
  const bool have = b < job.nblocks;
  if (have) {
    const ResampleBlock rb = traj[job.traj0 + b];
    const GA_GLOBAL float* __restrict in = gptr(job.buf) + job.start_pos;
    int64_t ip = rb.consumed;           // next input index (relative)
    double Pos = rb.pos;
    int ready = rb.ready;
    float S0 = 0.f, S1 = 0.f, S2 = 0.f, S3 = 0.f;
    // the window holds the last `ready` consumed samples (Shift, CubicResampler.cs:91-97)
    if (ready >= 1) S3 = in[ip - 1];
    if (ready >= 2) S2 = in[ip - 2];
    if (ready >= 3) S1 = in[ip - 3];
    if (ready >= 4) S0 = in[ip - 4];
    while (ready < 4 && ip < job.avail) {   // priming (:31-35)
      S0 = S1; S1 = S2; S2 = S3; S3 = in[ip++];
      ready++;
    }
    int outp = 0;
    if (ready == 4) {
      for (; outp < rb.produced; outp++) {
        int consume = (int)Pos;
        for (int i = 0; i < consume; i++) { S0 = S1; S1 = S2; S2 = S3; S3 = in[ip++]; }
        Pos -= consume;
        float t = (float)Pos;
        tile[lane][outp] = cubic_interp(S0, S1, S2, S3, t);
        Pos += job.rate;
      }
    }
    for (; outp < kBlock; outp++) tile[lane][outp] = 0.f;   // outputSpan.Slice(outIdx).Clear()
  }
  __syncthreads();
  const int nb = (int)min<int64_t>(64, job.nblocks - bl0);
  GA_GLOBAL float* __restrict out = gptr(job.out) + (job.b0 + bl0) * kBlock;
  store_tile(tile, out, nb, lane);
}
__global__ __launch_bounds__(256) void resample_fast_kernel(const ResampleFastJob* __restrict jobs) {
  const ResampleFastJob job = jobs[blockIdx.y];
  const int64_t total = job.nblocks * kBlock;
  const GA_GLOBAL float* __restrict in = gptr(job.buf) + job.start_pos;
  const GA_GLOBAL v2f* __restrict sm = (const GA_GLOBAL v2f*)job.samples;   // (ip as the bits of .x, t = .y: one 8-byte load)
  GA_GLOBAL float* __restrict out = gptr(job.out) + job.b0 * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const v2f e = sm[i];
    const GA_GLOBAL float* __restrict w = in + (int64_t)__float_as_uint(e.x) - 4;
    const float S0 = w[0], S1 = w[1], S2 = w[2], S3 = w[3];
    const float t = e.y;
    out[i] = cubic_interp(S0, S1, S2, S3, t);
  }
}
void launch_resample_fast(hipStream_t s, const ResampleFastJob* jobs_dev, int njobs, int64_t max_blocks) {
  if (njobs <= 0 || max_blocks <= 0) return;
  // (8 rounds per workgroup when there are thousands of jobs: 4096 voices x 469 one-round workgroups were bound by the dispatch rate)
  int rounds = 1;
  if (const char* e = expenv("GA_RS_ROUNDS")) rounds = std::max(1, atoi(e));
  else if ((int64_t)njobs * ((max_blocks * kBlock + 255) / 256) > 200000) rounds = 8;
  const int gx = (int)std::min<int64_t>((max_blocks * kBlock + 256 * rounds - 1) / (256 * rounds), 512);
  GA_LAUNCH_JOBS(resample_fast_kernel, gx, 256, jobs_dev, njobs);
}
void launch_resample(hipStream_t s, const ResampleJob* jobs_dev, int njobs, const ResampleBlock* traj_dev, int64_t max_blocks) {
  if (njobs <= 0 || max_blocks <= 0) return;
  int gx = (int)((max_blocks + 63) / 64);
  GA_LAUNCH_JOBS(resample_kernel, gx, 64, jobs_dev, njobs, traj_dev);
}


// =====================================================================================================
//  General source replay (see GsrBlock): one lane per block, fed samples gathered by index with the loop wrap rule
//  `pos >= loopEnd -> loopStart` (AudioBufferSourceNode.cs:262-265,297-314).  A rare path (looping + resampling,
//  moving playbackRate): gathers are uncoalesced, stores go through LDS like resample_kernel.
// =====================================================================================================
__global__ __launch_bounds__(64) void gsr_kernel(const GsrJob* __restrict jobs, const uint8_t* __restrict base) {
  __shared__ float tile[64][kBlock + 1];
  const GsrJob job = jobs[blockIdx.y];
  const int lane = threadIdx.x;
  const int64_t bl0 = (int64_t)blockIdx.x * 64;
  if (bl0 >= job.nblocks) return;
  const int64_t b = bl0 + lane;
  if (b < job.nblocks) {
    const GsrBlock d = (job.desc ? job.desc : (const GsrBlock*)(base + job.desc_off))[b];   // (`base` is a kernel argument: global)
    const GA_GLOBAL float* __restrict in = gptr(job.buf);
    int64_t ip = d.next;
    auto feed = [&]() {
      float v = in[ip++];
      if (job.loop && ip >= job.loop_end) ip = job.loop_start;
      return v;
    };
    int outp = 0;
    if (d.copy) {
      for (; outp < d.produced; outp++) tile[lane][outp] = feed();
    } else {
      float S0 = d.w[0] >= 0 ? in[d.w[0]] : 0.f, S1 = d.w[1] >= 0 ? in[d.w[1]] : 0.f;
      float S2 = d.w[2] >= 0 ? in[d.w[2]] : 0.f, S3 = d.w[3] >= 0 ? in[d.w[3]] : 0.f;
      double Pos = d.pos;
      int ready = d.ready;
      if (d.produced > 0) {
        while (ready < 4) {   // priming (CubicResampler.cs:31-35); the host has checked that the inputs exist
          S0 = S1; S1 = S2; S2 = S3; S3 = feed();
          ready++;
        }
        for (; outp < d.produced; outp++) {
          int consume = (int)Pos;
          for (int i = 0; i < consume; i++) { S0 = S1; S1 = S2; S2 = S3; S3 = feed(); }
          Pos -= consume;
          float t = (float)Pos;
          tile[lane][outp] = cubic_interp(S0, S1, S2, S3, t);
          Pos += d.rate;
        }
      }
    }
    for (; outp < kBlock; outp++) tile[lane][outp] = 0.f;
  }
  __syncthreads();
  const int nb = (int)min<int64_t>(64, job.nblocks - bl0);
  GA_GLOBAL float* __restrict out = gptr(job.out) + (job.b0 + bl0) * kBlock;
  store_tile(tile, out, nb, lane);
}
void launch_gsr(hipStream_t s, const GsrJob* jobs_dev, int njobs, const uint8_t* plan_base_dev, int64_t max_blocks) {
  if (njobs <= 0 || max_blocks <= 0) return;
  int gx = (int)((max_blocks + 63) / 64);
  GA_LAUNCH_JOBS(gsr_kernel, gx, 64, jobs_dev, njobs, plan_base_dev);
}


// =====================================================================================================
//  Modulated k-rate playbackRate (see KrateProbeJob, GsrWalkJob): the rate of every block, then the source walk
// =====================================================================================================
__global__ __launch_bounds__(64) void krate_probe_kernel(const KrateProbeJob* __restrict jobs, const uint8_t* __restrict base,
                                                         const double* __restrict bt, int64_t nblocks) {
  const KrateProbeJob job = jobs[blockIdx.y];
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= nblocks) return;
  const float* const* rows = (const float* const*)(base + job.rows_off);
  float v = param_value_at((const ParamEvent*)(base + job.events_off), job.nev, job.value, bt[b]);   // intrinsic value at the block start
  const float* row = rows[b];
  // Math.Clamp(intrinsicValue + modulation, min, max), except for a NaN: fmaxf turns it into the lower bound.  The reference converts a
  // NaN rate with (int) / (long) casts, which have no defined result to match, and the replay needs a finite rate.
  if (row) v = fminf(fmaxf(v + gptr(row)[b * kBlock], job.vmin), job.vmax);
  gptr(job.out)[b] = v;
}
void launch_krate_probe(hipStream_t s, const KrateProbeJob* jobs_dev, int njobs, const uint8_t* plan_base_dev, const double* block_times_dev,
                        int64_t nblocks) {
  if (njobs <= 0 || nblocks <= 0) return;
  int gx = (int)((nblocks + 63) / 64);
  GA_LAUNCH_JOBS(krate_probe_kernel, gx, 64, jobs_dev, njobs, plan_base_dev, block_times_dev, nblocks);
}

__global__ __launch_bounds__(64) void gsr_walk_kernel(const GsrWalkJob* __restrict jobs, int njobs) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= njobs) return;
  const GsrWalkJob job = jobs[i];
  GsrState st = job.st;
  int64_t endRel = -1;
  int err = GSR_OK;
  int64_t rel = 0;
  for (; rel < job.nrel && err == GSR_OK; rel++) {
    GsrBlock d;
    bool end = false;
    const int64_t b = job.bs + rel;
    int e = (b >= 0 && b < job.nrates) ? gsrReplayBlock(job.g, job.rates[b], st, d, end) : GSR_ERR_FEED;
    if (e == GSR_OK) {
      if (end && endRel < 0) endRel = rel;
      else if (!end && endRel >= 0) e = GSR_ERR_RESUMED;   // (with unchanged controls an END block is followed by END blocks only)
    }
    if (e == GSR_OK && endRel < 0) e = gsrCheckBlock(job.g, d);   // END blocks are cleared: no reads
    if (e != GSR_OK) {
      err = e;
      d.copy = 1;
      d.produced = 0;
      d.next = 0;
    }
    job.desc[rel] = d;
    if (endRel >= 0 && job.endsAtEnd) {
      rel++;
      break;
    }
  }
  for (; rel < job.nrel; rel++) {   // (after a failure: silence; the host refuses the chunk before anything reads these)
    GsrBlock d{};
    d.copy = 1;
    job.desc[rel] = d;
  }
  GsrBlock tail{};   // the state after the last walked block
  tail.pp = st.pp;
  for (int k = 0; k < 4; k++) tail.w[k] = st.w[k];
  tail.pos = st.pos;
  tail.ready = st.ready;
  job.desc[job.nrel] = tail;
  GsrWalkOut o;
  o.endRel = endRel;
  o.st = st;
  o.err = err;
  o.pad_ = 0;
  *job.out = o;
}
void launch_gsr_walk(hipStream_t s, const GsrWalkJob* jobs_dev, int njobs) {
  if (njobs <= 0) return;
  hipLaunchKernelGGL(gsr_walk_kernel, dim3((njobs + 63) / 64), dim3(64), 0, s, jobs_dev, njobs);
}


// =====================================================================================================
//  AudioStreamNodeBase.Process (see StreamPiece): one lane per block, pieces of a block in order; stores go through LDS like
//  resample_kernel.  A rare path (streams are few): gathers are per lane.
// =====================================================================================================
__global__ __launch_bounds__(64) void stream_kernel(const StreamJob* __restrict jobs, const uint8_t* __restrict base) {
  __shared__ float tile[64][kBlock + 1];
  const StreamJob job = jobs[blockIdx.y];
  const int lane = threadIdx.x;
  const int64_t bl0 = (int64_t)blockIdx.x * 64;
  if (bl0 >= job.nblocks) return;
  const StreamSeg* __restrict segs = (const StreamSeg*)(base + job.segs_off);
  const GA_GLOBAL float* win_in = gptr(job.win_in);
  auto sample = [&](int seg, int64_t idx) -> float {
    if (seg == -1) return 0.f;
    if (seg == -2) return win_in[idx];
    const StreamSeg sg = segs[seg];
    return ldg1(sg.base + (int64_t)job.ch * sg.stride + idx);
  };
  const int64_t b = bl0 + lane;
  if (b < job.nblocks) {
    const StreamBlock blk = ((const StreamBlock*)(base + job.blocks_off))[job.b0 + b];
    for (int i = 0; i < kBlock; i++) tile[lane][i] = 0.f;   // frames no piece covers are cleared
    for (int q = 0; q < blk.npieces; q++) {
      const StreamPiece d = ((const StreamPiece*)(base + job.pieces_off))[blk.piece0 + q];
      const StreamSeg sg = segs[d.seg];
      const GA_GLOBAL float* __restrict in = gptr(sg.base) + (int64_t)job.ch * sg.stride;
      int64_t ip = d.next;
      int outp = d.out0;
      const int oend = d.out0 + d.produced;
      if (d.copy) {
        for (; outp < oend; outp++) tile[lane][outp] = in[ip++];
      } else {
        float S0 = sample(d.wseg[0], d.w[0]), S1 = sample(d.wseg[1], d.w[1]);
        float S2 = sample(d.wseg[2], d.w[2]), S3 = sample(d.wseg[3], d.w[3]);
        double Pos = d.pos;
        int ready = d.ready;
        if (d.produced > 0) {
          while (ready < 4) {   // priming (CubicResampler.cs:31-35); the host has checked that the inputs exist
            S0 = S1; S1 = S2; S2 = S3; S3 = in[ip++];
            ready++;
          }
          for (; outp < oend; outp++) {
            int consume = (int)Pos;
            for (int i = 0; i < consume; i++) { S0 = S1; S1 = S2; S2 = S3; S3 = in[ip++]; }
            Pos -= consume;
            float t = (float)Pos;
            tile[lane][outp] = cubic_interp(S0, S1, S2, S3, t);
            Pos += d.rate;
          }
        }
      }
    }
  }
  __syncthreads();
  const int nb = (int)min<int64_t>(64, job.nblocks - bl0);
  GA_GLOBAL float* __restrict out = gptr(job.out) + (job.b0 + bl0) * kBlock;
  store_tile(tile, out, nb, lane);
  if (job.win_out && blockIdx.x == 0 && lane < 4) gptr(job.win_out)[lane] = sample(job.wend_seg[lane], job.wend[lane]);
}
void launch_stream(hipStream_t s, const StreamJob* jobs_dev, int njobs, const uint8_t* plan_base_dev, int64_t max_blocks) {
  if (njobs <= 0 || max_blocks <= 0) return;
  int gx = (int)((max_blocks + 63) / 64);
  GA_LAUNCH_JOBS(stream_kernel, gx, 64, jobs_dev, njobs, plan_base_dev);
}

// =====================================================================================================
//  ConstantSourceNode / OscillatorNode / StereoPannerNode (see ga_kernels.hpp)
// =====================================================================================================
__global__ __launch_bounds__(256) void const_source_kernel(const ConstJob* __restrict jobs) {
  const ConstJob job = jobs[blockIdx.y];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < job.n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = job.f0 + i;
    float v = 0.f;
    if (f >= job.lo && f < job.hi) v = job.curve ? gptr(job.curve)[f] : job.value;
    gptr(job.out)[f] = v;
  }
}
void launch_const_source(hipStream_t s, const ConstJob* jobs_dev, int njobs, int64_t max_n) {
  if (njobs <= 0 || max_n <= 0) return;
  int gx = (int)std::min<int64_t>((max_n + 255) / 256, 1024);
  GA_LAUNCH_JOBS(const_source_kernel, gx, 256, jobs_dev, njobs);
}

__device__ __forceinline__ float osc_sample(double ph, int type) {   // GenerateSample, OscillatorNode.cs:171-195
  const double PI = 3.14159265358979323846;
  switch (type) {
    case 0: return (float)sin(ph);
    case 1: return ph < PI ? 1.0f : -1.0f;
    case 2: return (float)(2.0 * (ph / (2.0 * PI)) - 1.0);
    case 3: {
      double t = ph / (2.0 * PI);
      return (float)(4.0 * fabs(t - floor(t + 0.5)) - 1.0);
    }
    default: return 0.f;
  }
}
__global__ __launch_bounds__(64) void oscillator_kernel(const OscJob* __restrict jobs) {
  extern __shared__ double osc_lds[];
  // [64] block-start phases | [64][129] floats: samples out | (curve jobs only) [64][128] doubles: phase increments
  double* start_ph = osc_lds;
  float (*tile)[kBlock + 1] = reinterpret_cast<float (*)[kBlock + 1]>(osc_lds + 64);
  double* incs = osc_lds + 64 + (64 * (kBlock + 1) * sizeof(float) + 7) / 8;
  const OscJob job = jobs[blockIdx.x];
  const int lane = threadIdx.x;
  const double PI2 = 2.0 * 3.14159265358979323846;
  const double sr = (double)job.sample_rate;
  const bool curve = job.curve != nullptr;
  const double inc_const = (PI2 * (double)job.value) / sr;   // `(2.0 * Math.PI * freqValues[i]) / Context.SampleRate` (:140)
  double ph = *gptr(job.phase);
  const int64_t nblk = job.n / kBlock;
  for (int64_t g0 = 0; g0 < nblk; g0 += 64) {
    const int nb = (int)min<int64_t>(64, nblk - g0);
    const int64_t fg = job.f0 + g0 * kBlock;   // first frame of this group of blocks
    if (curve) {   // the increments of the whole group, computed 64-wide (the division stays out of the serial chain)
      for (int r = 0; r < nb; r++) {
        const int64_t f = fg + (int64_t)r * kBlock;
        incs[r * kBlock + lane] = (PI2 * (double)gptr(job.curve)[f + lane]) / sr;
        incs[r * kBlock + 64 + lane] = (PI2 * (double)gptr(job.curve)[f + 64 + lane]) / sr;
      }
      __syncthreads();
    }
    if (lane == 0) {   // the serial recurrence (:139-143), only the phase: `_phase += inc; if (_phase >= 2 pi) _phase -= 2 pi`
      for (int r = 0; r < nb; r++) {
        start_ph[r] = ph;
        const int64_t f = fg + (int64_t)r * kBlock;
        if (f + kBlock <= job.lo || f >= job.hi) continue;
        const int i0 = (int)max<int64_t>(job.lo - f, 0), i1 = (int)min<int64_t>(job.hi - f, kBlock);
        if (curve) {
          for (int i = i0; i < i1; i++) {
            ph += incs[r * kBlock + i];
            if (ph >= PI2) ph -= PI2;
          }
        } else {
          for (int i = i0; i < i1; i++) {
            ph += inc_const;
            if (ph >= PI2) ph -= PI2;
          }
        }
      }
    }
    __syncthreads();
    if (lane < nb) {
      double p = start_ph[lane];
      const int64_t f = fg + (int64_t)lane * kBlock;
      for (int i = 0; i < kBlock; i++) {
        float v = 0.f;
        if (f + i >= job.lo && f + i < job.hi) {
          v = osc_sample(p, job.type);
          p += curve ? incs[lane * kBlock + i] : inc_const;
          if (p >= PI2) p -= PI2;
        }
        tile[lane][i] = v;
      }
    }
    __syncthreads();
    for (int r = 0; r < nb; r++) {
      GA_GLOBAL float* o = gptr(job.out) + fg + (int64_t)r * kBlock;
      o[lane] = tile[r][lane];
      o[64 + lane] = tile[r][64 + lane];
    }
    __syncthreads();
    ph = __shfl(ph, 0);   // every lane carries the running phase (only lane 0 advanced it)
  }
  if (lane == 0) *gptr(job.phase) = ph;
}
void launch_oscillator(hipStream_t s, const OscJob* jobs_dev, int njobs, bool any_curve) {
  if (njobs <= 0) return;
  size_t lds = 64 * sizeof(double) + ((64 * (kBlock + 1) * sizeof(float) + 7) / 8) * 8 + (any_curve ? 64 * kBlock * sizeof(double) : 0);
  if (lds > 48 * 1024)   // (a per-device attribute: set whenever it is needed, a process may drive several devices)
    (void)hipFuncSetAttribute((const void*)oscillator_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
  hipLaunchKernelGGL(oscillator_kernel, dim3(njobs), dim3(64), lds, s, jobs_dev);
}

__global__ __launch_bounds__(256) void stereo_panner_kernel(const PanJob* __restrict jobs) {
  const PanJob job = jobs[blockIdx.y];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < job.n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = job.f0 + i;
    if (!job.stereo) {   // ProcessMono, :103-105
      const float x = gptr(job.in_l)[f];
      gptr(job.out_l)[f] = x * job.gain_l;
      gptr(job.out_r)[f] = x * job.gain_r;
    } else {             // ProcessStereo, :135-145
      const float inl = gptr(job.in_l)[f], inr = gptr(job.in_r)[f];
      if (job.pan <= 0.0f) {
        gptr(job.out_l)[f] = inl + inr * job.gain_l;
        gptr(job.out_r)[f] = inr * job.gain_r;
      } else {
        gptr(job.out_l)[f] = inl * job.gain_l;
        gptr(job.out_r)[f] = inr + inl * job.gain_r;
      }
    }
  }
}
void launch_stereo_panner(hipStream_t s, const PanJob* jobs_dev, int njobs, int64_t max_n) {
  if (njobs <= 0 || max_n <= 0) return;
  int gx = (int)std::min<int64_t>((max_n + 255) / 256, 1024);
  GA_LAUNCH_JOBS(stereo_panner_kernel, gx, 256, jobs_dev, njobs);
}

__global__ __launch_bounds__(256) void delay_kernel(const DelayJob* __restrict jobs) {
  const DelayJob job = jobs[blockIdx.y];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < job.n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = job.f0 + i;
    const float dt = job.curve ? gptr(job.curve)[f] : job.value;
    int d = (int)(dt * (float)job.sample_rate);   // float * int -> float, truncated (:68, :88)
    d = min(max(d, 0), job.max_delay);
    gptr(job.out)[f] = d > 0 ? gptr(job.line)[f - d] : 0.f;
  }
}
void launch_delay(hipStream_t s, const DelayJob* jobs_dev, int njobs, int64_t max_n) {
  if (njobs <= 0 || max_n <= 0) return;
  int gx = (int)std::min<int64_t>((max_n + 255) / 256, 1024);
  GA_LAUNCH_JOBS(delay_kernel, gx, 256, jobs_dev, njobs);
}

// The first 128-frame block of a DelayNode's output rows that holds a sample `!= 0f` (see DelayOnsetJob).  One wave per block and
// turn: lane l tests frames l and l + 64 of every row (rows are 4-byte aligned in general: dword loads, coalesced), a ballot says
// whether the block holds one, lane 0 lowers the job's word.  A wave visits its blocks in rising order and stops at its first hit.
__global__ __launch_bounds__(256) void delay_onset_kernel(const DelayOnsetJob* __restrict jobs) {
  const DelayOnsetJob& job = jobs[blockIdx.y];   // (read in place: the row table is indexed in a loop)
  const int lane = threadIdx.x & 63;
  const int nrows = min(max(job.nrows, 0), kDelayOnsetRows);
  const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t b = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); b < job.count; b += waves) {
    const int64_t f = ((int64_t)job.first + b) * kBlock + lane;
    unsigned bits = 0;
    for (int r = 0; r < nrows; r++) {
      const GA_GLOBAL float* p = gptr(job.rows[r]) + f;
      // -0.0f is zero, a NaN and a denormal are not: the bit pattern without its sign, whatever the wave's denormal mode
      bits |= (__float_as_uint(p[0]) << 1) | (__float_as_uint(p[64]) << 1);
    }
    if (__ballot(bits != 0) != 0ull) {   // (wave-uniform: every lane leaves the loop)
      if (lane == 0) atomicMin(job.out, (int32_t)(job.first + b));
      break;
    }
  }
}
void launch_delay_onset(hipStream_t s, const DelayOnsetJob* jobs_dev, int njobs, int64_t max_blocks) {
  if (njobs <= 0 || max_blocks <= 0) return;
  int gx = (int)std::min<int64_t>((max_blocks + 3) / 4, 256);
  GA_LAUNCH_JOBS(delay_onset_kernel, gx, 256, jobs_dev, njobs);
}

// delay_kernel and delay_onset_kernel for one block in one launch (see DelayProbeJob): two waves, lane l of wave w computes frame
// 64 w + l, one ballot per wave, one lane per wave lowers the word and only on a hit.
__global__ __launch_bounds__(kBlock) void delay_probe_kernel(const DelayProbeJob* __restrict jobs) {
  const DelayProbeJob job = jobs[blockIdx.y];
  const int64_t f = job.f0 + threadIdx.x;
  const float dt = job.curve ? gptr(job.curve)[f] : job.value;
  int d = (int)(dt * (float)job.sample_rate);   // float * int -> float, truncated (:68, :88)
  d = min(max(d, 0), job.max_delay);
  const float v = d > 0 ? gptr(job.line)[f - d] : 0.f;
  gptr(job.out)[f] = v;
  // -0.0f is zero, a NaN and a denormal are not: the bit pattern without its sign, whatever the wave's denormal mode
  if (__ballot((__float_as_uint(v) << 1) != 0u) != 0ull && (threadIdx.x & 63) == 0) atomicMin(job.word, job.block);
}
void launch_delay_probe(hipStream_t s, const DelayProbeJob* jobs_dev, int njobs) {
  if (njobs <= 0) return;
  GA_LAUNCH_JOBS(delay_probe_kernel, 1, kBlock, jobs_dev, njobs);
}


template <bool LX>   // (option "libm_exact", as biquad_update_coefficients)
__device__ __forceinline__ void pan_gains(float pan, int stereo, float& gl, float& gr) {   // :94-98 / :129-133
  const float PIf = 3.14159265358979323846f;
  const float x = stereo ? (pan <= 0.0f ? pan + 1.0f : pan) : (pan + 1.0f) * 0.5f;
  const float a = x * PIf / 2.0f;
  gl = LX ? ga_cosf(a) : (float)cos((double)a);   // (rounded once from double: the C library's cosf / sinf behind MathF up to their last bit)
  gr = LX ? ga_sinf(a) : (float)sin((double)a);
}
template <bool LX>
__global__ __launch_bounds__(64) void stereo_panner_dynamic_kernel(const PanDynJob* __restrict jobs) {
  __shared__ float chg_pan[64];
  __shared__ int chg_has[64];
  __shared__ PanState carry[65];
  const PanDynJob job = jobs[blockIdx.x];
  const int lane = threadIdx.x;
  const GA_GLOBAL float* psrc = (const GA_GLOBAL float*)job.state;   // {last_pan, gain_l, gain_r, pad}
  PanState st = job.init ? job.init_state : PanState{psrc[0], psrc[1], psrc[2], psrc[3]};
  const int64_t nblk = job.n / kBlock;
  auto panAt = [&](int64_t f) { return clamp_ref(job.curve ? gptr(job.curve)[f] : job.value, -1.0f, 1.0f); };   // Math.Clamp(panValues[i], -1, 1)
  for (int64_t g0 = 0; g0 < nblk; g0 += 64) {
    const int nb = (int)min<int64_t>(64, nblk - g0);
    const int64_t fb = job.f0 + (g0 + lane) * kBlock;
    // last index of this block at which pan differs from the previous sample's pan (the previous sample of the block's first
    // frame is the last frame of the block before; for the job's very first frame it is the carried _lastPan)
    int has = 0;
    float cp = 0.f;
    if (lane < nb) {
      float prev = (g0 + lane == 0) ? st.last_pan : panAt(fb - 1);
      for (int i = 0; i < kBlock; i++) {
        const float p = panAt(fb + i);
        if (p != prev) { has = 1; cp = p; }   // NaN != NaN: a NaN _lastPan (initial state) forces the first computation
        prev = p;
      }
    }
    chg_has[lane] = has;
    chg_pan[lane] = cp;
    __syncthreads();
    if (lane == 0) {   // state at the start of every block of the group
      PanState cur = st;
      for (int r = 0; r < nb; r++) {
        carry[r] = cur;
        if (chg_has[r]) {
          cur.last_pan = chg_pan[r];
          pan_gains<LX>(cur.last_pan, job.stereo, cur.gain_l, cur.gain_r);
        }   // no change in the block: every pan of the block equals the carried _lastPan
      }
      carry[nb] = cur;
    }
    __syncthreads();
    if (lane < nb) {
      PanState s0 = carry[lane];
      float gl = s0.gain_l, gr = s0.gain_r, lp = s0.last_pan;
      for (int i = 0; i < kBlock; i++) {
        const int64_t f = fb + i;
        const float pan = panAt(f);
        if (pan != lp) {
          pan_gains<LX>(pan, job.stereo, gl, gr);
          lp = pan;
        }
        if (!job.stereo) {
          const float x = gptr(job.in_l)[f];
          gptr(job.out_l)[f] = x * gl;
          gptr(job.out_r)[f] = x * gr;
        } else {
          const float inl = gptr(job.in_l)[f], inr = gptr(job.in_r)[f];
          if (pan <= 0.0f) {
            gptr(job.out_l)[f] = inl + inr * gl;
            gptr(job.out_r)[f] = inr * gr;
          } else {
            gptr(job.out_l)[f] = inl * gl;
            gptr(job.out_r)[f] = inr + inl * gr;
          }
        }
      }
    }
    __syncthreads();
    st = carry[nb];
    __syncthreads();
  }
  if (lane == 0) {
    GA_GLOBAL float* pdst = (GA_GLOBAL float*)job.state;
    pdst[0] = st.last_pan; pdst[1] = st.gain_l; pdst[2] = st.gain_r; pdst[3] = st.pad_;
  }
}
void launch_stereo_panner_dynamic(hipStream_t s, const PanDynJob* jobs_dev, int njobs, bool libm_exact) {
  if (njobs <= 0) return;
  if (libm_exact) hipLaunchKernelGGL(stereo_panner_dynamic_kernel<true>, dim3(njobs), dim3(64), 0, s, jobs_dev);
  else hipLaunchKernelGGL(stereo_panner_dynamic_kernel<false>, dim3(njobs), dim3(64), 0, s, jobs_dev);
}


__global__ __launch_bounds__(256) void interleave_kernel(float* __restrict dst, InterleaveSrc src, int channels, int used, int64_t f0, int64_t n) {
  // one thread per output element: consecutive threads write consecutive floats (coalesced); the reads of one channel are
  // strided by `channels` across the wave and served from L2
  const int64_t total = n * channels;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = i / channels;
    const int ch = (int)(i - f * channels);
    dst[(f0 + f) * channels + ch] = ch < used ? src.ch[ch][f0 + f] : 0.f;
  }
}
void launch_interleave(hipStream_t s, float* dst, InterleaveSrc src, int channels, int used, int64_t f0, int64_t n) {
  if (n <= 0 || channels <= 0) return;
  int gx = (int)std::min<int64_t>((n * channels + 255) / 256, 4096);
  hipLaunchKernelGGL(interleave_kernel, dim3(gx), dim3(256), 0, s, dst, src, channels, used, f0, n);
}


__global__ __launch_bounds__(256) void param_mod_kernel(const ParamModJob* __restrict jobs) {
  const ParamModJob job = jobs[blockIdx.y];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < job.n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = job.f0 + i;
    const int64_t fs = job.krate ? f - (f % kBlock) : f;   // k-rate: `_input.Buffer.GetChannelSpan(0)[0]` and the block-start value
    const float intr = job.intrinsic ? gptr(job.intrinsic)[fs] : job.value;
    gptr(job.out)[f] = clamp_ref(intr + gptr(job.mod)[fs], job.vmin, job.vmax);   // Math.Clamp(intrinsicValue + modulation, min, max)
  }
}
void launch_param_mod(hipStream_t s, const ParamModJob* jobs_dev, int njobs, int64_t max_n) {
  if (njobs <= 0 || max_n <= 0) return;
  int gx = (int)std::min<int64_t>((max_n + 255) / 256, 1024);
  GA_LAUNCH_JOBS(param_mod_kernel, gx, 256, jobs_dev, njobs);
}

}  // namespace ga
