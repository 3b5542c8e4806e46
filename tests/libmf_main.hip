// Stand-alone device check of graphaudio_amd/csrc/ga_libmf.hpp (option "libm_exact"): one kernel evaluates ga_cosf / ga_sinf on about
// 2^24 arguments (every 64th float of [0, 4.0], the signs alternating, plus both signs of every float within 64 ulp of k pi / 4 for
// k = 0 .. 5, of 2^-12 and of 2 * 3.14159274f * 24000 / 48000), another ga_powf(10, y) on about 2^24 exponents (every 64th float of
// [0, 1.5], the signs alternating, plus y = fl(g / 40f) for 2^20 gains g of [-60, 60]).  The host evaluates the same header on the same
// arguments; the condition is identical bit patterns.  What the machine's libm computes plays no part here (tests/libmf_main.cpp).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "ga_libmf.hpp"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); std::exit(1); } } while (0)

__global__ __launch_bounds__(256) void trig_kernel(const float* __restrict x, float* __restrict c, float* __restrict s, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  c[i] = ga_cosf(x[i]);
  s[i] = ga_sinf(x[i]);
}
__global__ __launch_bounds__(256) void pow_kernel(const float* __restrict y, float* __restrict p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  p[i] = ga_powf(10.f, y[i]);
}

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

template <class T>
struct Dev {
  T* p = nullptr;
  size_t n;
  explicit Dev(size_t n_) : n(n_) { CK(hipMalloc(&p, n * sizeof(T))); CK(hipMemset(p, 0xCD, n * sizeof(T))); }
  ~Dev() { (void)hipFree(p); }
  Dev(const Dev&) = delete;
  Dev& operator=(const Dev&) = delete;
  void put(const std::vector<T>& h) { CK(hipMemcpy(p, h.data(), n * sizeof(T), hipMemcpyHostToDevice)); }
  std::vector<T> host() const {
    std::vector<T> h(n);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
    return h;
  }
};

template <class F>
static int compare(const char* name, const std::vector<float>& arg, const std::vector<float>& got, F host) {
  size_t bad = 0;
  for (size_t i = 0; i < arg.size(); i++)
    if (bits(got[i]) != bits(host(arg[i])) && !bad++)
      std::printf("%s: first difference at argument bits 0x%08x: device 0x%08x host 0x%08x\n", name, bits(arg[i]), bits(got[i]), bits(host(arg[i])));
  std::printf("%s %zu arguments, device != host: %zu\n", name, arg.size(), bad);
  return bad != 0;
}

int main() {
  std::vector<float> x;
  for (uint32_t b = 0, k = 0; b <= 0x40800000u; b += 64, k++) x.push_back(from_bits(b | (k & 1) << 31));
  {
    std::vector<float> centres;
    for (int k = 0; k <= 5; k++) centres.push_back((float)(k * (3.14159265358979323846 / 4)));
    centres.push_back(0x1p-12f);
    centres.push_back(2.f * 3.14159274f * 24000.f / 48000.f);
    for (float c : centres)
      for (int d = -64; d <= 64; d++) {
        const int64_t b = (int64_t)bits(c) + d;
        if (b >= 0) { x.push_back(from_bits((uint32_t)b)); x.push_back(-from_bits((uint32_t)b)); }
      }
  }
  std::vector<float> y;
  for (uint32_t b = 0, k = 0; b <= 0x3fc00000u; b += 64, k++) y.push_back(from_bits(b | (k & 1) << 31));
  for (int i = 0; i < (1 << 20); i++) y.push_back((float)(-60.0 + 120.0 * (double)i / (double)((1 << 20) - 1)) / 40.f);

  int fails = 0;
  {
    const int64_t n = (int64_t)x.size();
    Dev<float> dx(x.size()), dc(x.size()), ds(x.size());
    dx.put(x);
    hipLaunchKernelGGL(trig_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dx.p, dc.p, ds.p, n);
    CK(hipGetLastError());
    fails += compare("ga_cosf", x, dc.host(), [](float a) { return ga_cosf(a); });
    fails += compare("ga_sinf", x, ds.host(), [](float a) { return ga_sinf(a); });
  }
  {
    const int64_t n = (int64_t)y.size();
    Dev<float> dy(y.size()), dp(y.size());
    dy.put(y);
    hipLaunchKernelGGL(pow_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dy.p, dp.p, n);
    CK(hipGetLastError());
    fails += compare("ga_powf", y, dp.host(), [](float a) { return ga_powf(10.f, a); });
  }
  std::printf(fails ? "FAILED\n" : "ok\n");
  return fails ? 1 : 0;
}
