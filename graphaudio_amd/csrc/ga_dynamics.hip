// ga_dynamics.hip -- DynamicsCompressorNode (include/graphaudio_hip.h): compressor_kernel.  The node has no
// counterpart in the reference; the definition is this library's own and is held to a float64 model (tests/_compressor_model.py).
// Wave64, -ffp-contract=off: see ga_kernels.hip (every product and sum of the definition is rounded separately).

#include "ga_kernels.hpp"
#include "ga_device_common.hpp"

#include <hip/hip_runtime.h>

namespace ga {

// lane `lane` (wave-uniform) of v, in every lane: two v_readlane_b32
__device__ __forceinline__ double compressor_bcast(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// steps 1 - 4 of the definition for one frame: a = max over channels of |x| (exact in float), widened
__device__ __forceinline__ double compressor_xl(float a, const CompressorParams& p) {
  const double ad = (double)a;
  if (ad < p.quiet) return 0.0;   // 2 (xG - T) < -W with room to spare (CompressorParams::quiet): yG = xG, xL = xG - xG = +0
  const double xG = 20.0 * log10(ad > 1e-6 ? ad : 1e-6);
  const double d = xG - p.T;
  double yG;
  if (2.0 * d < -p.W) {
    yG = xG;
  } else if (p.W > 0.0 && fabs(2.0 * d) <= p.W) {
    const double q = d + p.W / 2.0;
    yG = xG + ((1.0 / p.R - 1.0) * (q * q)) / (2.0 * p.W);
  } else {
    yG = p.T + d / p.R;
  }
  return xG - yG;
}

// =====================================================================================================
//  One workgroup = one wavefront = one job (a node over consecutive segments of a chunk).  Per tile of 64 frames:
//    1. lane l: xL of frame l (log10 and the knee: the expensive part, 64 wide), and the two products (1 - aA) xL, (1 - aR) xL
//       the recurrence adds -- they do not depend on yL
//    2. the recurrence, 64 steps, wave-uniform: xL[i] and its two products come by v_readlane (the lane index is a constant of the
//       unrolled loop); every lane evaluates both branches aA yL + pA, aR yL + pR beside the comparison and selects -- the chain per
//       frame is a product, a sum and a select -- and lane i keeps the yL of step i
//    3. lane l: g = (float)pow(10, (M - yL) / 20), y_c = x_c g
//  The next tile's samples are loaded in front of step 1, so their latency runs under the walk.  A silent segment (nch = 0) has
//  xL = 0: yL is multiplied by aR per frame while it is positive, a yL of 0 stays (the segment is skipped), and a yL below 0 (a
//  rounding residue of xG - (T + d / R) at R = 1) takes the general walk, whose comparison then picks the attack branch as the
//  definition does.  No LDS, no atomics; the only writes are the outputs of the job's own segments and its yL.
// =====================================================================================================
__global__ __launch_bounds__(64) void compressor_kernel(const CompressorJob* __restrict jobs, const uint8_t* __restrict tables) {
  const CompressorJob job = jobs[blockIdx.x];
  const CompressorSeg* segs = (const CompressorSeg*)(tables + job.seg_off);
  const CompressorParams* pars = (const CompressorParams*)(tables + job.par_off);
  const int lane = threadIdx.x;
  double yl = *job.state;
  for (int s = 0; s < job.nseg; s++) {
    const CompressorSeg sg = segs[s];
    const int nch = sg.nch;
    if (nch == 0 && yl == 0.0) continue;
    if (nch == 0 && yl > 0.0) {   // (xL = 0 <= yL: the release branch, aR yL + (1 - aR) 0 = aR yL, and the value stays >= 0)
      for (int b = 0; b < sg.nb && yl != 0.0; b++) {
        const double aR = pars[(sg.b0 + b) * job.par_stride].aR;
        for (int i = 0; i < kBlock; i++) yl = aR * yl;
      }
      continue;
    }
    const float* in0 = sg.in[0];
    const float* in1 = sg.in[1];
    const int ntiles = 2 * sg.nb;
    int64_t f = (int64_t)sg.b0 * kBlock + lane;
    float n0 = 0.f, n1 = 0.f;
    if (nch >= 1) n0 = in0[f];
    if (nch == 2) n1 = in1[f];
    for (int t = 0; t < ntiles; t++, f += 64) {
      const float x0 = n0, x1 = n1;
      if (t + 1 < ntiles) {
        if (nch >= 1) n0 = in0[f + 64];
        if (nch == 2) n1 = in1[f + 64];
      }
      const CompressorParams p = pars[(sg.b0 + (t >> 1)) * job.par_stride];
      const float a = nch == 2 ? fmaxf(fabsf(x0), fabsf(x1)) : fabsf(x0);
      const double xl = nch ? compressor_xl(a, p) : 0.0;
      const double pa = (1.0 - p.aA) * xl, pr = (1.0 - p.aR) * xl;
      double mine = 0.0;
#pragma unroll
      for (int i = 0; i < 64; i++) {
        const double xi = compressor_bcast(xl, i), pai = compressor_bcast(pa, i), pri = compressor_bcast(pr, i);
        const double ua = p.aA * yl + pai, ur = p.aR * yl + pri;
        yl = xi > yl ? ua : ur;
        if (lane == i) mine = yl;
      }
      if (nch) {
        const float g = (float)pow(10.0, (p.M - mine) / 20.0);
        sg.out[0][f] = x0 * g;
        if (nch == 2) sg.out[1][f] = x1 * g;
      }
    }
  }
  if (lane == 0) *job.state = yl;
}

void launch_compressor(hipStream_t s, const CompressorJob* jobs_dev, int njobs, const uint8_t* tables_dev) {
  if (njobs <= 0) return;
  hipLaunchKernelGGL(compressor_kernel, dim3(njobs), dim3(64), 0, s, jobs_dev, tables_dev);
}

}  // namespace ga
