// Stand-alone run of the seven 256-point real-FFT kernels of the convolver path (graphaudio_amd/csrc/ga_rfft.hip) through their
// launchers alone: rfft_fwd_kernel, rfft_fwd_b_kernel<double|float>, conv_rebuild_kernel, irfft_ola_kernel and
// irfft_ola_b_kernel<double|float>.  Inputs come from a seeded integer generator; every output array of every case is printed as one
// FNV-1a 64-bit digest ("digest <name> <hex>"), and tests/test_gpu_rfft_kernels.py compares them with tests/golden/rfft_kernel_digests.json,
// recorded while every kernel still carried its own copy of the transform.  Two identities are checked element by element ("identity <name> ok|FAIL"):
//   1. forward A, forward B<double> and conv_rebuild give the same spectra for the same blocks,
//   2. inverse A and inverse B<double> give the same samples and the same outgoing overlap.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ga_kernels.hpp"

using namespace ga;

namespace ga {
[[noreturn]] void launch_fail(const char* what) {   // (ga_engine.cpp's is not linked here)
  std::printf("launch_fail: %s\n", what);
  std::exit(2);
}
}  // namespace ga

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); std::exit(1); } } while (0)

static int identityFailures = 0;

struct Rng {   // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  float unit() { return (float)((double)(int64_t)(next() >> 40) / 8388608.0 - 1.0); }   // 24 bits -> [-1, 1), exact
};

static uint64_t fnv1a(const void* p, size_t n) {
  const unsigned char* b = (const unsigned char*)p;
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001b3ull; }
  return h;
}
static void digest(const std::string& name, const std::vector<float>& v) {
  std::printf("digest %s %016llx\n", name.c_str(), (unsigned long long)fnv1a(v.data(), v.size() * 4));
}
static void identity(const std::string& name, size_t bad, size_t n) {
  std::printf("identity %s %s (%zu of %zu differ)\n", name.c_str(), bad ? "FAIL" : "ok", bad, n);
  if (bad) identityFailures++;
}
static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

template <class T>
struct Dev {   // device array; outputs start as the byte 0xCD everywhere, so an element nobody wrote shows in the digest
  T* p = nullptr;
  size_t n;
  explicit Dev(size_t n_) : n(n_ ? n_ : 1) { CK(hipMalloc(&p, n * sizeof(T))); CK(hipMemset(p, 0xCD, n * sizeof(T))); }
  explicit Dev(const std::vector<T>& h) : Dev(h.size()) { if (!h.empty()) CK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice)); }
  ~Dev() { (void)hipFree(p); }
  Dev(const Dev&) = delete;
  Dev& operator=(const Dev&) = delete;
  std::vector<T> host() const {
    std::vector<T> h(n);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
    return h;
  }
};

static int roundup(int n, int m) { return (n + m - 1) / m * m; }

// row kinds of the 33-row cases: row 3 has no buffer, row 5 is all zeros, row 7 is scaled by 1e-30
enum { kRowNull = 3, kRowZero = 5, kRowTiny = 7 };
static float row_scale(int nrows, int row) { return nrows > 1 && row == kRowZero ? 0.f : nrows > 1 && row == kRowTiny ? 1e-30f : 1.f; }

static Twiddles gTw;

// ---- forward: A, B<double>, B<float> on the same signals; returns B<double>'s planes for the rebuild comparison ----------------
struct FwdB { std::vector<float> xr, xi; int hist, tx; };
static FwdB forward_case(const std::string& tag, const std::vector<float>& sig, const std::vector<char>& isNull, int nrows, int n, bool withA) {
  const int hist = 4, tx = hist + roundup(n, 16) + 16, ty = roundup(n, 256), rp = 128;
  Dev<float> dsig(sig);
  std::vector<ConvRowIO> io(nrows);
  for (int r = 0; r < nrows; r++) io[r] = ConvRowIO{isNull[r] ? nullptr : dsig.p + (size_t)r * n * kBlock, nullptr};
  Dev<ConvRowIO> dio(io);
  FwdB res{{}, {}, hist, tx};
  std::vector<float> axr, axi;
  if (withA) {
    Dev<float> xr((size_t)kBins * tx * rp), xi((size_t)kBins * tx * rp);
    launch_rfft_fwd(0, dio.p, nrows, n, hist, ConvPlanes{xr.p, xi.p, nullptr, nullptr, tx, ty, rp}, gTw);
    CK(hipGetLastError());
    axr = xr.host();
    axi = xi.host();
    digest("fwd_a." + tag + ".xr", axr);
    digest("fwd_a." + tag + ".xi", axi);
  }
  for (int fp64 = 1; fp64 >= 0; fp64--) {
    Dev<float> xr((size_t)nrows * kBins * tx), xi((size_t)nrows * kBins * tx);
    launch_rfft_fwd_b(0, dio.p, nrows, n, hist, ConvPlanesB{xr.p, xi.p, nullptr, nullptr, tx, ty}, gTw, fp64 != 0);
    CK(hipGetLastError());
    std::vector<float> hr = xr.host(), hi = xi.host();
    if (withA) {
      digest(std::string(fp64 ? "fwd_b64." : "fwd_b32.") + tag + ".xr", hr);
      digest(std::string(fp64 ? "fwd_b64." : "fwd_b32.") + tag + ".xi", hi);
    }
    if (fp64) { res.xr = hr; res.xi = hi; }
  }
  if (withA) {
    size_t bad = 0, cnt = 0;
    for (int r = 0; r < nrows; r++)
      for (int k = 0; k < kBins; k++)
        for (int t = 0; t < n; t++, cnt++) {
          const size_t a = ((size_t)k * tx + hist + t) * rp + r, b = ((size_t)r * kBins + k) * tx + hist + t;
          if (!same(axr[a], res.xr[b]) || !same(axi[a], res.xi[b])) bad++;
        }
    identity("fwd_a_eq_b64." + tag, bad, cnt);
  }
  return res;
}

static std::vector<float> make_signal(Rng& rng, int nrows, int n) {
  std::vector<float> sig((size_t)nrows * n * kBlock);
  for (int r = 0; r < nrows; r++) {
    const float sc = row_scale(nrows, r);
    for (int i = 0; i < n * kBlock; i++) sig[(size_t)r * n * kBlock + i] = rng.unit() * sc;
  }
  return sig;
}

static void forward_cases() {
  for (int nrows : {1, 33})
    for (int n : {1, 15, 16, 17, 31, 32, 33, 65}) {
      Rng rng{(uint64_t)(1000 * nrows + n)};
      std::vector<float> sig = make_signal(rng, nrows, n);
      std::vector<char> isNull(nrows, 0);
      if (nrows > 1) isNull[kRowNull] = 1;
      forward_case("r" + std::to_string(nrows) + ".n" + std::to_string(n), sig, isNull, nrows, n, true);
    }
}

// ---- conv_rebuild: jobs of P, P (no source) and ceil(P / 2) blocks in one launch, against B<double> on the same blocks ----------
static void rebuild_cases() {
  for (int P : {1, 2, 32, 33, 70}) {
    const std::string tag = "p" + std::to_string(P);
    const int hist = conv_rebuild_hist(P), tx = conv_rebuild_tx(P);
    const int jobP[3] = {P, P, (P + 1) / 2};
    Rng rng{(uint64_t)(77000 + P)};
    std::vector<float> sig = make_signal(rng, 3, P);   // job j reads the first jobP[j] blocks of row j
    for (size_t i = 0; i < (size_t)P * kBlock; i++) sig[2 * (size_t)P * kBlock + i] *= 1e-30f;
    Dev<float> dsig(sig);
    const size_t sstride = (size_t)kBins * (P > 1 ? P - 1 : 1);
    Dev<float> sr(3 * sstride), si(3 * sstride), xr((size_t)3 * kBins * tx), xi((size_t)3 * kBins * tx);
    std::vector<ConvRebuildJob> jobs(3);
    for (int j = 0; j < 3; j++)
      jobs[j] = ConvRebuildJob{j == 1 ? nullptr : dsig.p + (size_t)j * P * kBlock, sr.p + j * sstride, si.p + j * sstride, jobP[j], j};
    Dev<ConvRebuildJob> djobs(jobs);
    launch_conv_rebuild(0, djobs.p, 3, P, ConvPlanesB{xr.p, xi.p, nullptr, nullptr, tx, kRebuildTy}, hist, gTw);
    CK(hipGetLastError());
    std::vector<float> hxr = xr.host(), hxi = xi.host(), hsr = sr.host(), hsi = si.host();
    digest("rebuild." + tag + ".xr", hxr);
    digest("rebuild." + tag + ".xi", hxi);
    digest("rebuild." + tag + ".store_r", hsr);
    digest("rebuild." + tag + ".store_i", hsi);
    size_t bad = 0, cnt = 0;
    for (int j = 0; j < 3; j++) {
      const int Pj = jobP[j];
      std::vector<float> one(sig.begin() + (size_t)j * P * kBlock, sig.begin() + ((size_t)j * P + Pj) * kBlock);
      FwdB b = forward_case("", one, std::vector<char>(1, j == 1), 1, Pj, false);
      for (int k = 0; k < kBins; k++)
        for (int t = 0; t < Pj; t++, cnt++) {
          const size_t bo = (size_t)k * b.tx + b.hist + t, po = conv_rebuild_plane_index(j, tx, hist, Pj, k, t);
          bool ok = same(hxr[po], b.xr[bo]) && same(hxi[po], b.xi[bo]);
          if (t >= 1) {
            const size_t so = j * sstride + conv_rebuild_store_index(Pj, k, t);
            ok = ok && same(hsr[so], b.xr[bo]) && same(hsi[so], b.xi[bo]);
          }
          if (!ok) bad++;
        }
    }
    identity("rebuild_eq_b64." + tag, bad, cnt);
  }
}

// ---- inverse: A, B<double>, B<float> on the same spectra, two consecutive chunks ------------------------------------------------
static void inverse_cases() {
  for (int nrows : {1, 33})
    for (int n : {1, 15, 16, 17, 31, 32, 33, 65}) {
      const std::string tag = "r" + std::to_string(nrows) + ".n" + std::to_string(n);
      const int tx = 4 + roundup(n, 16) + 16, ty = roundup(n, 256), rp = 128;
      Rng rng{(uint64_t)(500000 + 1000 * nrows + n)};
      const size_t outN = (size_t)nrows * n * kBlock, ovN = (size_t)nrows * kBlock;
      std::vector<float> outA, outB[2], ovA[2], ovB[2][2];   // [fp64][chunk]
      Dev<float> aout(2 * outN), aov0(std::vector<float>(ovN, 0.f)), aov1(ovN), aov2(ovN);
      Dev<float> bout0(2 * outN), bout1(2 * outN);
      Dev<float> bov00(std::vector<float>(ovN, 0.f)), bov01(ovN), bov02(ovN), bov10(std::vector<float>(ovN, 0.f)), bov11(ovN), bov12(ovN);
      float* aovs[3] = {aov0.p, aov1.p, aov2.p};
      float* bouts[2] = {bout0.p, bout1.p};
      float* bovs[2][3] = {{bov00.p, bov01.p, bov02.p}, {bov10.p, bov11.p, bov12.p}};
      for (int chunk = 0; chunk < 2; chunk++) {
        // spectra [row][bin][block] over the whole y extent, and the same values as [bin][block][row]
        std::vector<float> byr((size_t)nrows * kBins * ty), byi(byr.size()), ayr((size_t)kBins * ty * rp, 0.f), ayi(ayr.size(), 0.f);
        for (int r = 0; r < nrows; r++) {
          const float sc = row_scale(nrows, r);
          for (int k = 0; k < kBins; k++)
            for (int t = 0; t < ty; t++) {
              const size_t b = ((size_t)r * kBins + k) * ty + t, a = ((size_t)k * ty + t) * rp + r;
              ayr[a] = byr[b] = rng.unit() * sc;
              ayi[a] = byi[b] = rng.unit() * sc;
            }
        }
        std::vector<ConvRowIO> aio(nrows);
        for (int r = 0; r < nrows; r++)
          aio[r] = ConvRowIO{nullptr, nrows > 1 && r == kRowNull ? nullptr : aout.p + ((size_t)chunk * nrows + r) * n * kBlock};
        Dev<ConvRowIO> daio(aio);
        Dev<float> dayr(ayr), dayi(ayi), dbyr(byr), dbyi(byi);
        launch_irfft_ola(0, daio.p, nrows, n, ConvPlanes{nullptr, nullptr, dayr.p, dayi.p, tx, ty, rp}, aovs[chunk], aovs[chunk + 1], gTw);
        CK(hipGetLastError());
        for (int fp64 = 0; fp64 < 2; fp64++) {
          std::vector<ConvRowIO> bio(nrows);
          std::vector<const float*> oin(nrows);
          std::vector<float*> oout(nrows);
          for (int r = 0; r < nrows; r++) {
            bio[r] = ConvRowIO{nullptr, nrows > 1 && r == kRowNull ? nullptr : bouts[fp64] + ((size_t)chunk * nrows + r) * n * kBlock};
            oin[r] = bovs[fp64][chunk] + (size_t)r * kBlock;
            oout[r] = bovs[fp64][chunk + 1] + (size_t)r * kBlock;
          }
          Dev<ConvRowIO> dbio(bio);
          Dev<const float*> doin(oin);
          Dev<float*> doout(oout);
          launch_irfft_ola_b(0, dbio.p, nrows, n, ConvPlanesB{nullptr, nullptr, dbyr.p, dbyi.p, tx, ty}, doin.p, doout.p, gTw, fp64 != 0);
          CK(hipGetLastError());
          CK(hipDeviceSynchronize());
        }
        CK(hipDeviceSynchronize());
      }
      outA = aout.host();
      ovA[0] = aov1.host();
      ovA[1] = aov2.host();
      digest("inv_a." + tag + ".out", outA);
      digest("inv_a." + tag + ".overlap1", ovA[0]);
      digest("inv_a." + tag + ".overlap2", ovA[1]);
      for (int fp64 = 1; fp64 >= 0; fp64--) {
        outB[fp64] = (fp64 ? bout1 : bout0).host();
        ovB[fp64][0] = (fp64 ? bov11 : bov01).host();
        ovB[fp64][1] = (fp64 ? bov12 : bov02).host();
        const std::string nm = fp64 ? "inv_b64." : "inv_b32.";
        digest(nm + tag + ".out", outB[fp64]);
        digest(nm + tag + ".overlap1", ovB[fp64][0]);
        digest(nm + tag + ".overlap2", ovB[fp64][1]);
      }
      size_t bad = 0, cnt = 0;
      for (size_t i = 0; i < 2 * outN; i++, cnt++) bad += !same(outA[i], outB[1][i]);
      for (int c = 0; c < 2; c++)
        for (size_t i = 0; i < ovN; i++, cnt++) bad += !same(ovA[c][i], ovB[1][c][i]);
      identity("inv_a_eq_b64." + tag, bad, cnt);
    }
}

int main() {
  // twiddle tables as the engine computes them (ga_engine.cpp, Context::init_device)
  const double pi = 3.14159265358979323846264338327950288;
  std::vector<double2> t128(64), t256(129);
  for (int j = 0; j < 64; j++) t128[j] = make_double2(std::cos(2.0 * pi * j / 128.0), -std::sin(2.0 * pi * j / 128.0));
  for (int k = 0; k <= 128; k++) t256[k] = make_double2(std::cos(2.0 * pi * k / 256.0), -std::sin(2.0 * pi * k / 256.0));
  Dev<double2> d128(t128), d256(t256);
  gTw = Twiddles{d128.p, d256.p};
  forward_cases();
  rebuild_cases();
  inverse_cases();
  CK(hipDeviceSynchronize());
  std::printf("identities failed: %d\n", identityFailures);
  return 0;
}
