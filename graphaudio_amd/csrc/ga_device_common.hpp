// ga_device_common.hpp -- the few device-side definitions that more than one kernel file (ga_kernels.hip, ga_conv.hip,
// ga_spatial.hip) uses.  Include from .hip translation units only; the host/device contract is ga_kernels.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

namespace ga {

// gridDim.y is limited to 65535: a level of a fragmented chunk (thousands of voices x tens of segments) can hold more jobs than
// that, so every (x = frames, y = job) launcher walks the job table in windows.  Kernels index `jobs[blockIdx.y]`.
constexpr int kMaxGridY = 32768;
#define GA_LAUNCH_JOBS(kernel, gx_, block_, jobs_, njobs_, ...)                                                      \
  for (int j0_ = 0; j0_ < (njobs_); j0_ += kMaxGridY)                                                                \
    hipLaunchKernelGGL(kernel, dim3((gx_), std::min(kMaxGridY, (njobs_) - j0_)), dim3(block_), 0, s, (jobs_) + j0_, ##__VA_ARGS__)

typedef float f32x4 __attribute__((ext_vector_type(4)));

}  // namespace ga
