// ga_rfft.hip -- the 256-point real FFT of the convolver path: one wavefront transform core and the five kernels that stage
// data into and out of it (formulation A: rfft_fwd_kernel / irfft_ola_kernel; formulations B, C, R and the conv_migrate rebuild:
// rfft_fwd_b_kernel / conv_rebuild_kernel / irfft_ola_b_kernel).  The arithmetic -- casts, in-lane stage, the six cross-lane
// stages, the real-FFT split and un-split, the 1/256 scale -- is written once, in rfft256_fwd and rfft256_inv; a kernel owns only
// where its floats come from, its staging layout in LDS, its global loads and stores and its overlap handling.  One exception, for a
// measured reason: irfft_ola_b_kernel carries the statements of rfft256_inv inline (see there).
// Compiled with -ffp-contract=off (see ga_kernels.hip): fused multiply-adds appear only where fma() is written.

#include "ga_kernels.hpp"
#include "ga_fft16.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace ga {

// phase timestamps for tools/micro/rfft_phase.hip (compiled out of the product)
#ifdef GA_EXP_TIMELINE
__device__ unsigned long long* ga_tl = nullptr;
#define GA_TL(i) do { if (ga_tl && threadIdx.x == 0) ga_tl[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 8 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define GA_TL(i) do { } while (0)
#endif

// =====================================================================================================
//  256-point real FFT on one wavefront (forward: RealFourierTransform.cs:62-88; inverse: :101-131), double precision.
//  z[n] = x[2n] + i x[2n+1] (n < 128); lane l owns z[l] (slot 0) and z[l+64] (slot 1).  One in-lane radix-2 stage
//  and six cross-lane stages; the cross-lane exchanges are DPP moves (xor 1,2,4,8), ds_swizzle (xor 16) and one
//  ds_bpermute (xor 32) -- no LDS storage, no barriers.  Butterflies are select-free: every lane evaluates
//  d = fma(sigma, mine, partner) followed by one complex multiply whose twiddle is (1, 0) on the "lower" lanes.
//  Each wavefront keeps N independent transforms in flight to hide the exchange latency.
// =====================================================================================================
template <int MASK>
__device__ __forceinline__ int xchg32(int v) {
  if constexpr (MASK == 1) return __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true);           // quad_perm [1,0,3,2]
  else if constexpr (MASK == 2) return __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, true);      // quad_perm [2,3,0,1]
  else if constexpr (MASK == 4) {                                                                // xor 7 then xor 3
    int t = __builtin_amdgcn_mov_dpp(v, 0x141, 0xF, 0xF, true);                                  // row_half_mirror
    return __builtin_amdgcn_mov_dpp(t, 0x1B, 0xF, 0xF, true);                                    // quad_perm [3,2,1,0]
  } else if constexpr (MASK == 8) {                                                              // xor 15 then xor 7
    int t = __builtin_amdgcn_mov_dpp(v, 0x140, 0xF, 0xF, true);                                  // row_mirror
    return __builtin_amdgcn_mov_dpp(t, 0x141, 0xF, 0xF, true);
  } else if constexpr (MASK == 16) return __builtin_amdgcn_ds_swizzle(v, 0x401F);                // bit mode: xor 0x10
  else return __shfl_xor(v, MASK, 64);
}
template <int MASK>
__device__ __forceinline__ double xchg(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  return __hiloint2double(xchg32<MASK>(hi), xchg32<MASK>(lo));
}
template <int MASK>
__device__ __forceinline__ float xchg(float v) { return __int_as_float(xchg32<MASK>(__float_as_int(v))); }
__device__ __forceinline__ double shfl_d(double v, int src) { return __shfl(v, src, 64); }
__device__ __forceinline__ float shfl_d(float v, int src) { return __shfl(v, src, 64); }
__device__ __forceinline__ int rev6(int l) { return (int)(__brev((unsigned)l) >> 26); }

// T = double reproduces the reference's double-precision FftFlat transform (spectra equal after the float32 cast with
// overwhelming probability); T = float is the default fast path: the transform error (~1e-7 relative) stays an order of
// magnitude inside the float32 accumulation noise of the partition sum that follows.
template <class T>
struct LaneTwT {   // per-lane constants, loaded once per kernel by load_lane_tw
  T c[6], s[6];    // stage twiddle for half = 32,16,8,4,2,1: W128^{(l & (half-1)) * 64/half} on upper lanes, (1,0) on lower
  T sg[6];         // -1 on upper lanes (l & half), +1 on lower lanes
  T c1, s1;        // W128^l  (the in-lane stage)
  // after the DIF stages slot j of lane l holds Z[k], k = 2 m + j, m = rev6(l).  X[k] needs Z[128 - k]:
  //   j = 0: index 2 ((64 - m) & 63) -> lane src0 = rev6((64 - m) & 63) ; j = 1: index 2 (63 - m) + 1 -> lane src1 = 63 - l
  int m, src0, src1;
  T wk0x, wk0y;    // W256^(2m)      (the split / un-split of bin 2m)
  T wk1x, wk1y;    // W256^(2m + 1)
};
template <class T>
__device__ __forceinline__ LaneTwT<T> load_lane_tw(Twiddles tw, int lane) {
  LaneTwT<T> t;
#pragma unroll
  for (int i = 0; i < 6; i++) {
    int half = 32 >> i;
    bool up = (lane & half) != 0;
    double2 w = tw.w128[(lane & (half - 1)) * (64 / half)];
    t.c[i] = up ? (T)w.x : (T)1.0;
    t.s[i] = up ? (T)w.y : (T)0.0;
    t.sg[i] = up ? (T)-1.0 : (T)1.0;
  }
  double2 w = tw.w128[lane];
  t.c1 = (T)w.x;
  t.s1 = (T)w.y;
  t.m = rev6(lane);
  t.src0 = rev6((64 - t.m) & 63);
  t.src1 = 63 - lane;
  t.wk0x = (T)tw.w256[2 * t.m].x, t.wk0y = (T)tw.w256[2 * t.m].y;
  t.wk1x = (T)tw.w256[2 * t.m + 1].x, t.wk1y = (T)tw.w256[2 * t.m + 1].y;
  return t;
}
// decimation in frequency: lower <- a + b ; upper <- (a - b) W   (natural order in, bit-reversed out)
template <int HALF, int IDX, class T>
__device__ __forceinline__ void dif_stage(T& ar, T& ai, const LaneTwT<T>& t) {
  T pr = xchg<HALF>(ar), pi = xchg<HALF>(ai);
  T dr = fma(t.sg[IDX], ar, pr), di = fma(t.sg[IDX], ai, pi);   // lower: mine + partner ; upper: partner - mine
  ar = fma(dr, t.c[IDX], -(di * t.s[IDX]));
  ai = fma(dr, t.s[IDX], di * t.c[IDX]);
}
// decimation in time with conjugated twiddles: lower <- a + b conj(W) ; upper <- a - b conj(W)  (bit-reversed in, natural out)
template <int HALF, int IDX, class T>
__device__ __forceinline__ void dit_stage(T& ar, T& ai, const LaneTwT<T>& t) {
  T qr = fma(ar, t.c[IDX], ai * t.s[IDX]);       // mine * conj(tw)   (tw = (1,0) on lower lanes)
  T qi = fma(ai, t.c[IDX], -(ar * t.s[IDX]));
  T pr = xchg<HALF>(qr), pi = xchg<HALF>(qi);
  ar = fma(t.sg[IDX], qr, pr);                   // lower: a + q_partner ; upper: partner - q_mine
  ai = fma(t.sg[IDX], qi, pi);
}
// one cross-lane stage of all N transforms before any of them enters the next
template <int HALF, int IDX, int N, class T>
__device__ __forceinline__ void dif_row(T (&s0r)[N], T (&s0i)[N], T (&s1r)[N], T (&s1i)[N], const LaneTwT<T>& t) {
#pragma unroll
  for (int u = 0; u < N; u++) { dif_stage<HALF, IDX>(s0r[u], s0i[u], t); dif_stage<HALF, IDX>(s1r[u], s1i[u], t); }
}
template <int HALF, int IDX, int N, class T>
__device__ __forceinline__ void dit_row(T (&s0r)[N], T (&s0i)[N], T (&s1r)[N], T (&s1i)[N], const LaneTwT<T>& t) {
#pragma unroll
  for (int u = 0; u < N; u++) { dit_stage<HALF, IDX>(s0r[u], s0i[u], t); dit_stage<HALF, IDX>(s1r[u], s1i[u], t); }
}

// real-FFT split: X[k] = E[k] + W256^k * (-i) * D[k],  E = (Z[k] + conj Z[128-k]) / 2,  D = (Z[k] - conj Z[128-k]) / 2
template <class T>
__device__ __forceinline__ void rfft_split(T ax, T ay, int src, T wx, T wy, float& xr, float& xi) {
  T bx = shfl_d(ax, src), by = shfl_d(ay, src);
  T er = (T)0.5 * (ax + bx), ei = (T)0.5 * (ay - by);
  T dr = (T)0.5 * (ax - bx), di = (T)0.5 * (ay + by);
  T pr = fma(dr, wx, -(di * wy)), pi = fma(dr, wy, di * wx);
  xr = (float)(er + pi);   // T -> float, PartitionedConvolver.cs:117-118
  xi = (float)(ei - pr);
}
// its inverse: Z[k] = (X[k] + conj X[128-k]) + i conj(W256^k) (X[k] - conj X[128-k]), a = X[k], b = conj X[128-k]
template <class T>
__device__ __forceinline__ void rfft_unsplit(T ar, T ai, T br, T bi, T wx, T wy, T& zr, T& zi) {
  T er = ar + br, ei = ai + bi, dr = ar - br, di = ai - bi;
  T pr = fma(dr, wx, di * wy), pi = fma(di, wx, -(dr * wy));   // d * conj(w)
  zr = er - pi;
  zi = ei + pr;
}

struct RfftBins {              // what one lane holds of one spectrum, m = rev6(lane)
  float x0r, x0i, x1r, x1i;    // bins 2m (DC on the lane with m == 0: purely real) and 2m + 1
};
// forward transforms of N blocks: lane l brings samples 2l and 2l + 1 of each (xa, xb).  The lane with m == 0 also hands
// nyquist(u, X[128]) the Nyquist bin, Re Z[0] - Im Z[0], purely real like DC (RealFourierTransform.cs:76-78); the caller stores it
// there, inside this one branch: as a fifth output stored later it costs kernel A 40 VGPRs and a wave of occupancy.
template <int N, class T, class Nyq>
__device__ __forceinline__ void rfft256_fwd(const float* xa, const float* xb, const LaneTwT<T>& t, RfftBins (&X)[N], Nyq nyquist) {
  T s0r[N], s0i[N], s1r[N], s1i[N];
#pragma unroll
  for (int u = 0; u < N; u++) {
    s0r[u] = (T)xa[u];   // float -> T, PartitionedConvolver.cs:106
    s0i[u] = (T)xb[u];
    // in-lane stage with the zero upper half (PartitionedConvolver.cs:107): (a + 0, (a - 0) * W128^l)
    s1r[u] = fma(s0r[u], t.c1, -(s0i[u] * t.s1));
    s1i[u] = fma(s0r[u], t.s1, s0i[u] * t.c1);
  }
  dif_row<32, 0>(s0r, s0i, s1r, s1i, t);
  dif_row<16, 1>(s0r, s0i, s1r, s1i, t);
  dif_row<8, 2>(s0r, s0i, s1r, s1i, t);
  dif_row<4, 3>(s0r, s0i, s1r, s1i, t);
  dif_row<2, 4>(s0r, s0i, s1r, s1i, t);
  dif_row<1, 5>(s0r, s0i, s1r, s1i, t);
#pragma unroll
  for (int u = 0; u < N; u++) {
    rfft_split(s0r[u], s0i[u], t.src0, t.wk0x, t.wk0y, X[u].x0r, X[u].x0i);
    if (t.m == 0) {
      X[u].x0i = 0.f;
      nyquist(u, (float)(s0r[u] - s0i[u]));
    }
    rfft_split(s1r[u], s1i[u], t.src1, t.wk1x, t.wk1y, X[u].x1r, X[u].x1i);
  }
}

struct IrfftBins {   // what one lane reads of one spectrum, m = rev6(lane)
  float ar, ai, br, bi;   // bins 2m, 128 - 2m
  float cr, ci, dr, di;   // bins 2m + 1, 127 - 2m
};
struct IrfftSamples {
  float h0, h1, g0, g1;   // time samples 2l, 2l + 1 (head), 128 + 2l, 128 + 2l + 1 (tail)
};
// inverse transforms of N spectra
template <int N, class T>
__device__ __forceinline__ void rfft256_inv(const IrfftBins (&X)[N], const LaneTwT<T>& t, IrfftSamples (&y)[N]) {
  T s0r[N], s0i[N], s1r[N], s1i[N];
#pragma unroll
  for (int u = 0; u < N; u++) {   // float -> T, PartitionedConvolver.cs:136
    T ai = X[u].ai, bi = -(T)X[u].bi;
    if (t.m == 0) { ai = (T)0.0; bi = (T)0.0; }   // rdft ignores Im of DC / Nyquist (RealFourierTransform.cs:120-123)
    rfft_unsplit<T>(X[u].ar, ai, X[u].br, bi, t.wk0x, t.wk0y, s0r[u], s0i[u]);
    rfft_unsplit<T>(X[u].cr, X[u].ci, X[u].dr, -(T)X[u].di, t.wk1x, t.wk1y, s1r[u], s1i[u]);
  }
  dit_row<1, 5>(s0r, s0i, s1r, s1i, t);
  dit_row<2, 4>(s0r, s0i, s1r, s1i, t);
  dit_row<4, 3>(s0r, s0i, s1r, s1i, t);
  dit_row<8, 2>(s0r, s0i, s1r, s1i, t);
  dit_row<16, 1>(s0r, s0i, s1r, s1i, t);
  dit_row<32, 0>(s0r, s0i, s1r, s1i, t);
#pragma unroll
  for (int u = 0; u < N; u++) {
    // in-lane stage: z[l] = s0 + s1 conj(W128^l), z[l+64] = s0 - s1 conj(W128^l); scale 2/n * 1/2 (:46,129)
    T qr = fma(s1r[u], t.c1, s1i[u] * t.s1), qi = fma(s1i[u], t.c1, -(s1r[u] * t.s1));
    const T scale = (T)(1.0 / 256.0);
    y[u].h0 = (float)((s0r[u] + qr) * scale);
    y[u].h1 = (float)((s0i[u] + qi) * scale);
    y[u].g0 = (float)((s0r[u] - qr) * scale);
    y[u].g1 = (float)((s0i[u] - qi) * scale);
  }
}

// =====================================================================================================
//  Formulation A: planes [bin][block][row], row index fastest.
// =====================================================================================================
constexpr int FFT_ROWS = 32;        // rows (channel-instances) per workgroup
constexpr int STAGE_LD = 132;       // staging tile is [row][bin], bins fastest, 129 padded to 132 floats
constexpr int FFT_ILP = 4;          // independent transforms in flight per wavefront

// ---- forward ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rfft_fwd_kernel(const ConvRowIO* __restrict rows, int nrows, int nblocks, int hist,
                                                       ConvPlanes pl, Twiddles tw) {
  __shared__ float st_r[FFT_ROWS * STAGE_LD];
  __shared__ float st_i[FFT_ROWS * STAGE_LD];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rowtile = blockIdx.x;
  const int t = blockIdx.y;
  const LaneTwT<double> ltw = load_lane_tw<double>(tw, lane);
  const int k0 = 2 * ltw.m, k1 = 2 * ltw.m + 1;

  for (int q0 = 0; q0 < FFT_ROWS / 4; q0 += FFT_ILP) {
    float xa[FFT_ILP], xb[FFT_ILP];
#pragma unroll
    for (int u = 0; u < FFT_ILP; u++) {
      const int row = rowtile * FFT_ROWS + wave * (FFT_ROWS / 4) + q0 + u;
      const float* in = row < nrows ? rows[row].in : nullptr;
      xa[u] = 0.f;
      xb[u] = 0.f;
      if (in) {
        const GA_GLOBAL float* p = gptr(in) + (int64_t)t * kBlock + 2 * lane;
        xa[u] = p[0];
        xb[u] = p[1];
      }
    }
    RfftBins X[FFT_ILP];
    rfft256_fwd<FFT_ILP>(xa, xb, ltw, X, [&](int u, float nyq) {
      st_r[(wave * (FFT_ROWS / 4) + q0 + u) * STAGE_LD + 128] = nyq;
      st_i[(wave * (FFT_ROWS / 4) + q0 + u) * STAGE_LD + 128] = 0.f;
    });
#pragma unroll
    for (int u = 0; u < FFT_ILP; u++) {
      const int rl = wave * (FFT_ROWS / 4) + q0 + u;
      st_r[rl * STAGE_LD + k0] = X[u].x0r;
      st_i[rl * STAGE_LD + k0] = X[u].x0i;
      st_r[rl * STAGE_LD + k1] = X[u].x1r;
      st_i[rl * STAGE_LD + k1] = X[u].x1i;
    }
  }
  __syncthreads();
  // coalesced 16-byte stores: 8 lanes cover the 32 consecutive rows (one 128-byte line) of one bin
  const size_t plane_t = (size_t)pl.tx * pl.rp;
  const size_t base = (size_t)(hist + t) * pl.rp + (size_t)rowtile * FFT_ROWS;
  for (int idx = tid; idx < kBins * (FFT_ROWS / 4); idx += 256) {
    int k = idx / (FFT_ROWS / 4), r4 = (idx % (FFT_ROWS / 4)) * 4;
    size_t o = (size_t)k * plane_t + base + r4;
    float4 vr = make_float4(st_r[(r4 + 0) * STAGE_LD + k], st_r[(r4 + 1) * STAGE_LD + k], st_r[(r4 + 2) * STAGE_LD + k], st_r[(r4 + 3) * STAGE_LD + k]);
    float4 vi = make_float4(st_i[(r4 + 0) * STAGE_LD + k], st_i[(r4 + 1) * STAGE_LD + k], st_i[(r4 + 2) * STAGE_LD + k], st_i[(r4 + 3) * STAGE_LD + k]);
    *reinterpret_cast<float4*>(pl.xr + o) = vr;
    *reinterpret_cast<float4*>(pl.xi + o) = vi;
  }
}

void launch_rfft_fwd(hipStream_t s, const ConvRowIO* rows_dev, int nrows, int nblocks, int hist, ConvPlanes pl, Twiddles tw) {
  if (nrows <= 0 || nblocks <= 0) return;
  dim3 grid((nrows + FFT_ROWS - 1) / FFT_ROWS, nblocks);
  hipLaunchKernelGGL(rfft_fwd_kernel, grid, dim3(256), 0, s, rows_dev, nrows, nblocks, hist, pl, tw);
}

// ---- inverse + overlap-add ----------------------------------------------------------------------------
constexpr int OLA_RUN = 16;   // consecutive blocks per workgroup (one extra inverse FFT recovers the incoming tail)

__global__ __launch_bounds__(256) void irfft_ola_kernel(const ConvRowIO* __restrict rows, int nrows, int nblocks, ConvPlanes pl,
                                                        const float* __restrict overlap_in, float* __restrict overlap_out, Twiddles tw) {
  __shared__ float ys_r[FFT_ROWS * STAGE_LD];
  __shared__ float ys_i[FFT_ROWS * STAGE_LD];
  __shared__ float tail[FFT_ROWS][kBlock];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rowtile = blockIdx.x;
  const int ta = blockIdx.y * OLA_RUN;
  const int tb = min(ta + OLA_RUN, nblocks);
  const LaneTwT<double> ltw = load_lane_tw<double>(tw, lane);
  const int k0 = ltw.m << 1, k1 = k0 | 1;
  const size_t plane_t = (size_t)pl.ty * pl.rp;

  if (ta == 0) {  // incoming overlap of the chunk's first block = persistent _overlap (PartitionedConvolver.cs:28,148-149)
    for (int idx = tid; idx < FFT_ROWS * kBlock; idx += 256) {
      int r = idx / kBlock, i = idx % kBlock;
      int row = rowtile * FFT_ROWS + r;
      tail[r][i] = row < nrows ? overlap_in[(size_t)row * kBlock + i] : 0.f;
    }
  }
  for (int t = (ta == 0 ? 0 : ta - 1); t < tb; t++) {
    const bool pre = t < ta;   // only recompute block ta-1 to obtain its second half
    __syncthreads();
    const size_t base = (size_t)t * pl.rp + (size_t)rowtile * FFT_ROWS;
    for (int idx = tid; idx < kBins * (FFT_ROWS / 4); idx += 256) {   // 16-byte loads, 8 lanes per 128-byte bin line
      int k = idx / (FFT_ROWS / 4), r4 = (idx % (FFT_ROWS / 4)) * 4;
      size_t o = (size_t)k * plane_t + base + r4;
      float4 vr = *reinterpret_cast<const float4*>(pl.yr + o);
      float4 vi = *reinterpret_cast<const float4*>(pl.yi + o);
      ys_r[(r4 + 0) * STAGE_LD + k] = vr.x; ys_r[(r4 + 1) * STAGE_LD + k] = vr.y;
      ys_r[(r4 + 2) * STAGE_LD + k] = vr.z; ys_r[(r4 + 3) * STAGE_LD + k] = vr.w;
      ys_i[(r4 + 0) * STAGE_LD + k] = vi.x; ys_i[(r4 + 1) * STAGE_LD + k] = vi.y;
      ys_i[(r4 + 2) * STAGE_LD + k] = vi.z; ys_i[(r4 + 3) * STAGE_LD + k] = vi.w;
    }
    __syncthreads();
    for (int q0 = 0; q0 < FFT_ROWS / 4; q0 += FFT_ILP) {
      IrfftBins X[FFT_ILP];
#pragma unroll
      for (int u = 0; u < FFT_ILP; u++) {
        const float* cr = ys_r + (wave * (FFT_ROWS / 4) + q0 + u) * STAGE_LD;
        const float* ci = ys_i + (wave * (FFT_ROWS / 4) + q0 + u) * STAGE_LD;
        X[u] = IrfftBins{cr[k0], ci[k0], cr[128 - k0], ci[128 - k0], cr[k1], ci[k1], cr[128 - k1], ci[128 - k1]};
      }
      IrfftSamples y[FFT_ILP];
      rfft256_inv<FFT_ILP>(X, ltw, y);
#pragma unroll
      for (int u = 0; u < FFT_ILP; u++) {
        const int rl = wave * (FFT_ROWS / 4) + q0 + u;
        const int row = rowtile * FFT_ROWS + rl;
        if (row < nrows) {
          if (!pre) {
            float* out = rows[row].out;
            float o0 = y[u].h0 + tail[rl][2 * lane];        // (float)y[i] + overlap[i]  (:148)
            float o1 = y[u].h1 + tail[rl][2 * lane + 1];
            if (out) {
              *reinterpret_cast<GA_GLOBAL v2f*>(gptr(out) + (int64_t)t * kBlock + 2 * lane) = v2f{o0, o1};
            }
          }
          tail[rl][2 * lane] = y[u].g0;                      // overlap[i] = (float)y[i + 128]  (:149)
          tail[rl][2 * lane + 1] = y[u].g1;
        }
      }
    }
  }
  if (tb == nblocks) {
    __syncthreads();
    for (int idx = tid; idx < FFT_ROWS * kBlock; idx += 256) {
      int r = idx / kBlock, i = idx % kBlock;
      int row = rowtile * FFT_ROWS + r;
      if (row < nrows) overlap_out[(size_t)row * kBlock + i] = tail[r][i];
    }
  }
}

void launch_irfft_ola(hipStream_t s, const ConvRowIO* rows_dev, int nrows, int nblocks, ConvPlanes pl, const float* overlap_in,
                      float* overlap_out, Twiddles tw) {
  if (nrows <= 0 || nblocks <= 0) return;
  dim3 grid((nrows + FFT_ROWS - 1) / FFT_ROWS, (nblocks + OLA_RUN - 1) / OLA_RUN);
  hipLaunchKernelGGL(irfft_ola_kernel, grid, dim3(256), 0, s, rows_dev, nrows, nblocks, pl, overlap_in, overlap_out, tw);
}

// =====================================================================================================
//  Formulation B kernels (see ga_kernels.hpp): planes [row][bin][block], block index fastest.
// =====================================================================================================
constexpr int FB_RUN = 32;            // blocks per workgroup in the B-layout FFT kernels: 32 blocks = one 128-byte line per bin
// Staging tile [block][bin] in LDS (64 banks of 4 bytes).  A lane of the 128-point transforms owns bins (2m, 2m + 1) with
// m = rev6(lane) and needs their mirrors (128 - 2m, 127 - 2m): with the bins in natural order every one of those accesses
// is a 2-way bank conflict (64 lanes on the even or the odd banks only).  So a column keeps its even bins packed in
// E[0..64] (bin 2e at e) and its odd bins in O[0..63] (bin 2o + 1 at FB_OB + o): all four accesses become 4-byte operations
// whose 64 lanes hit 64 different banks (m, 64 - m, FB_OB + m, FB_OB + 63 - m are permutations of the banks).
// FB_OB == 4 (mod 8) and FB_KP == 18 (mod 64) keep the transposed side conflict-free too: a wave covers 8 consecutive bins
// (banks b..b+3 from E, b+4..b+7 from O) of 8 columns 4 apart (4 * FB_KP == 8 mod 64).
constexpr int FB_OB = 68;
constexpr int FB_KP = 146;
__device__ __forceinline__ int fb_pos(int k) { return (k & 1) * FB_OB + (k >> 1); }

// One run of 32 blocks of one signal -> the staging tile [block of the run][bin]: wave w transforms blocks w, w+4, ..., w+28 of the
// run, 4 in flight.  `in` holds `nblocks` blocks (nullptr: silence); blocks from `nblocks` on are zeros.
template <class T>
__device__ __forceinline__ void rfft_fwd_b_run(const GA_GLOBAL float* in, int t0, int nblocks, const LaneTwT<T>& ltw, float* st_r,
                                               float* st_i, int lane, int wave) {
  // all eight input blocks of this wave are requested up front: their HBM latency overlaps the first batch of transforms
  float inr[FB_RUN / 4], ini[FB_RUN / 4];
#pragma unroll
  for (int q = 0; q < FB_RUN / 4; q++) {
    const int t = t0 + wave + 4 * q;
    inr[q] = 0.f;
    ini[q] = 0.f;
    if (in && t < nblocks) {
      const GA_GLOBAL float* p = in + (int64_t)t * kBlock + 2 * lane;
      inr[q] = p[0];
      ini[q] = p[1];
    }
  }
  const int m = ltw.m;
#pragma unroll
  for (int bq = 0; bq < FB_RUN / 16; bq++) {
    RfftBins X[4];
    rfft256_fwd<4>(inr + bq * 4, ini + bq * 4, ltw, X, [&](int u, float nyq) {
      st_r[(wave + 4 * (bq * 4 + u)) * FB_KP + 64] = nyq;   // bin 128 = E[64]
      st_i[(wave + 4 * (bq * 4 + u)) * FB_KP + 64] = 0.f;
    });
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int tl = wave + 4 * (bq * 4 + u);   // block within the run
      st_r[tl * FB_KP + m] = X[u].x0r;          // bin 2m
      st_i[tl * FB_KP + m] = X[u].x0i;
      st_r[tl * FB_KP + FB_OB + m] = X[u].x1r;  // bin 2m + 1
      st_i[tl * FB_KP + FB_OB + m] = X[u].x1i;
    }
  }
}

// forward: workgroup = (x-row, run of 32 blocks)
template <class T>
__global__ __launch_bounds__(256) void rfft_fwd_b_kernel(const ConvRowIO* __restrict xrows, int nx, int nblocks, int hist,
                                                         ConvPlanesB pl, Twiddles tw, int row0) {
  // staging tile [block of the run][bin] in the even/odd layout described at FB_KP
  __shared__ __attribute__((aligned(16))) float st_r[FB_RUN * FB_KP];
  __shared__ __attribute__((aligned(16))) float st_i[FB_RUN * FB_KP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // consecutive workgroups take consecutive runs of ONE row: their 128-byte pieces of every bin line are adjacent in HBM
  const int xrow = row0 + blockIdx.y;
  const int t0 = blockIdx.x * FB_RUN;
  const LaneTwT<T> ltw = load_lane_tw<T>(tw, lane);
  const GA_GLOBAL float* in = gptr(xrows[xrow].in);
  GA_TL(0);
  rfft_fwd_b_run<T>(in, t0, nblocks, ltw, st_r, st_i, lane, wave);
  GA_TL(1);
  __syncthreads();
  GA_TL(2);
  // store: per bin 32 consecutive blocks = 128 bytes, 8 lanes x 16 B
  const size_t rowbase = (size_t)xrow * kBins * pl.tx + hist + t0;
  for (int idx = tid; idx < kBins * 8; idx += 256) {
    int k = idx >> 3, q = (idx & 7) * 4;
    if (t0 + q >= nblocks) continue;
    size_t o = rowbase + (size_t)k * pl.tx + q;
    const int pk = q * FB_KP + fb_pos(k);
    *reinterpret_cast<float4*>(pl.xr + o) = make_float4(st_r[pk], st_r[pk + FB_KP], st_r[pk + 2 * FB_KP], st_r[pk + 3 * FB_KP]);
    *reinterpret_cast<float4*>(pl.xi + o) = make_float4(st_i[pk], st_i[pk + FB_KP], st_i[pk + 2 * FB_KP], st_i[pk + 3 * FB_KP]);
  }
  GA_TL(3);
}
void launch_rfft_fwd_b(hipStream_t s, const ConvRowIO* xrows_dev, int nx, int nblocks, int hist, ConvPlanesB pl, Twiddles tw, bool fp64) {
  if (nx <= 0 || nblocks <= 0) return;
  for (int r0 = 0; r0 < nx; r0 += 65535) {   // gridDim.y limit
    dim3 grid((nblocks + FB_RUN - 1) / FB_RUN, std::min(65535, nx - r0));
    if (fp64) hipLaunchKernelGGL(rfft_fwd_b_kernel<double>, grid, dim3(256), 0, s, xrows_dev, nx, nblocks, hist, pl, tw, r0);
    else hipLaunchKernelGGL(rfft_fwd_b_kernel<float>, grid, dim3(256), 0, s, xrows_dev, nx, nblocks, hist, pl, tw, r0);
  }
}

// Option "conv_migrate": the spectra history of a convolver that leaves formulation D, rebuilt from D's input history (ga_conv_rebuild.hpp).
// Workgroup = (job, run of 32 blocks) on a source that is a plain run of P x 128 samples.  The spectra are the floats formulation R's
// forward transform would have written because both kernels call rfft_fwd_b_run<double>.  Each value goes to the scratch plane (all P
// blocks: the partition sum of block T-1 reads them) and to the node's [129][P-1] store (blocks T-P+1 .. T-1).
__global__ __launch_bounds__(256) void conv_rebuild_kernel(const ConvRebuildJob* __restrict jobs, ConvPlanesB pl, int hist, Twiddles tw,
                                                           int job0) {
  __shared__ __attribute__((aligned(16))) float st_r[FB_RUN * FB_KP];
  __shared__ __attribute__((aligned(16))) float st_i[FB_RUN * FB_KP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const ConvRebuildJob* __restrict Jp = &jobs[job0 + blockIdx.y];
  const int P = Jp->P, xrow = Jp->xrow;
  const int t0 = blockIdx.x * FB_RUN;
  if (t0 >= P) return;   // (uniform: the grid is sized for the longest job)
  const LaneTwT<double> ltw = load_lane_tw<double>(tw, lane);
  const GA_GLOBAL float* in = gptr(Jp->src);
  rfft_fwd_b_run<double>(in, t0, P, ltw, st_r, st_i, lane, wave);
  __syncthreads();
  // store: a wave writes the 32 blocks of two bins -- runs of 128 bytes in the plane, and in the store where P - 1 allows
  float* __restrict dr_ = Jp->dst_r;
  float* __restrict di_ = Jp->dst_i;
  for (int idx = tid; idx < kBins * FB_RUN; idx += 256) {
    const int k = idx >> 5, q = idx & (FB_RUN - 1);
    const int j = t0 + q;
    if (j >= P) continue;
    const int pk = q * FB_KP + fb_pos(k);
    const float vr = st_r[pk], vi = st_i[pk];
    const size_t po = conv_rebuild_plane_index(xrow, pl.tx, hist, P, k, j);
    pl.xr[po] = vr;
    pl.xi[po] = vi;
    if (j >= 1) {
      const size_t so = conv_rebuild_store_index(P, k, j);
      dr_[so] = vr;
      di_[so] = vi;
    }
  }
}
void launch_conv_rebuild(hipStream_t s, const ConvRebuildJob* jobs_dev, int njobs, int max_P, ConvPlanesB pl, int hist, Twiddles tw) {
  if (njobs <= 0 || max_P <= 0) return;
  for (int j0 = 0; j0 < njobs; j0 += 65535) {   // gridDim.y limit
    dim3 grid((max_P + FB_RUN - 1) / FB_RUN, std::min(65535, njobs - j0));
    hipLaunchKernelGGL(conv_rebuild_kernel, grid, dim3(256), 0, s, jobs_dev, pl, hist, tw, j0);
  }
}

// inverse + overlap-add, B layout: workgroup = (y-row, run of 32 blocks).  All 33 inverse transforms of the run (the extra
// one recovers the tail of the block before the run) are independent: 4 waves x 2 batches of 4, and the 33rd alone on one
// wave.  Heads and tails land in LDS, then
// out[t] = (float)head[t] + tail[t-1] is written as one contiguous, fully coalesced 16 KB range.
// This kernel carries the statements of rfft256_inv inline (un-split through rfft_unsplit, DIT rows, in-lane stage, scale), with a
// batch size NU = 4 or 1 that is a constant only after unrolling: through rfft256_inv<4> / <1> its transform phase measured 5 %
// (double) to 15 % (float) longer and the kernel 1-2 % (tools/micro/rfft_phase.hip).  tests/test_gpu_rfft_kernels.py holds it to
// irfft_ola_kernel's samples (which go through rfft256_inv) bit for bit: edit the two together.
template <class T>
__global__ __launch_bounds__(256) void irfft_ola_b_kernel(const ConvRowIO* __restrict yrows, int ny, int nblocks, ConvPlanesB pl,
                                                          const float* const* __restrict overlap_in, float* const* __restrict overlap_out,
                                                          Twiddles tw, int row0) {
  // staging tile [33 columns][bin] (even/odd layout, see FB_KP): column c <-> block ta - 1 + c ; the memory is reused for
  // the head/tail tiles afterwards
  constexpr int NC = FB_RUN + 1;
  __shared__ __attribute__((aligned(16))) float smem[2 * NC * FB_KP];   // 9636 floats >= (33 + 33) * 128 = 8448
  float* sr = smem;
  float* si = smem + NC * FB_KP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = row0 + blockIdx.y;
  const int ta = blockIdx.x * FB_RUN;
  const int tb = min(ta + FB_RUN, nblocks);
  const int nrun = tb - ta;
  const LaneTwT<T> ltw = load_lane_tw<T>(tw, lane);
  const T wk0x = ltw.wk0x, wk0y = ltw.wk0y, wk1x = ltw.wk1x, wk1y = ltw.wk1y;
  const float* __restrict yr = pl.yr + (size_t)row * kBins * pl.ty;
  const float* __restrict yi = pl.yi + (size_t)row * kBins * pl.ty;
  GA_TL(0);
  // columns 1..nrun <- blocks ta .. tb-1 (16-byte loads, 8 lanes per 128-byte bin line); column 0 <- block ta - 1
  {
    // all global loads of the tile first (10 x 16 B in flight per thread), then the LDS transposition: one exposed HBM latency
    // per workgroup instead of one per loop iteration
    constexpr int NIT = (kBins * 8 + 255) / 256;   // 5
    float4 vr[NIT], vi[NIT];
#pragma unroll
    for (int it = 0; it < NIT; it++) {
      const int idx = tid + 256 * it;
      const int k = idx >> 3, q = (idx & 7) * 4;
      vr[it] = make_float4(0.f, 0.f, 0.f, 0.f);
      vi[it] = vr[it];
      if (idx < kBins * 8 && ta + q < nblocks) {
        vr[it] = *reinterpret_cast<const float4*>(yr + (size_t)k * pl.ty + ta + q);
        vi[it] = *reinterpret_cast<const float4*>(yi + (size_t)k * pl.ty + ta + q);
      }
    }
#pragma unroll
    for (int it = 0; it < NIT; it++) {
      const int idx = tid + 256 * it;
      const int k = idx >> 3, q = (idx & 7) * 4;
      if (idx < kBins * 8) {
        const int pk = (1 + q) * FB_KP + fb_pos(k);
        sr[pk] = vr[it].x; sr[pk + FB_KP] = vr[it].y; sr[pk + 2 * FB_KP] = vr[it].z; sr[pk + 3 * FB_KP] = vr[it].w;
        si[pk] = vi[it].x; si[pk + FB_KP] = vi[it].y; si[pk + 2 * FB_KP] = vi[it].z; si[pk + 3 * FB_KP] = vi[it].w;
      }
    }
  }
  if (tid < kBins) {
    float vr = 0.f, vi = 0.f;
    if (ta > 0) {
      vr = yr[(size_t)tid * pl.ty + ta - 1];
      vi = yi[(size_t)tid * pl.ty + ta - 1];
    }
    sr[fb_pos(tid)] = vr;
    si[fb_pos(tid)] = vi;
  }
  GA_TL(1);
  __syncthreads();
  GA_TL(2);
  // transform columns c = 0..nrun (c = 0 only when ta > 0); results kept in registers until the staging tile is dead.
  // Batches 0 and 1: column (4 * bq + u) * 4 + wave ; batch 2: column 32 alone, on wave (run & 3) -- which wave takes it
  // rotates with the run, so the extra work spreads over the SIMDs.  (As a fifth transform of batch 1 it costs 50 more
  // VGPRs and a wave of occupancy: slower.)
  const int m = ltw.m;
  float hd[3][4][2], tl[3][4][2];
#pragma unroll
  for (int bq = 0; bq < 3; bq++) {
    constexpr int kFull = 4;
    const int NU = bq < 2 ? kFull : 1;
    const bool act = bq < 2 ? (bq * 16 <= nrun) : (wave == (int)(blockIdx.x & 3) && nrun == FB_RUN);   // wave uniform
#pragma unroll
    for (int u = 0; u < kFull; u++) hd[bq][u][0] = hd[bq][u][1] = tl[bq][u][0] = tl[bq][u][1] = 0.f;
    if (act) {
      T s0r[kFull], s0i[kFull], s1r[kFull], s1i[kFull];
#pragma unroll
      for (int u = 0; u < NU; u++) {
        const int c = bq < 2 ? (bq * 4 + u) * 4 + wave : FB_RUN;
        const float* cr = sr + c * FB_KP;
        const float* ci = si + c * FB_KP;
        {
          T ar = cr[m], ai = ci[m];                               // bin 2m
          T br = cr[64 - m], bi = -(T)ci[64 - m];                 // bin 128 - 2m
          if (m == 0) { ai = (T)0.0; bi = (T)0.0; }
          rfft_unsplit(ar, ai, br, bi, wk0x, wk0y, s0r[u], s0i[u]);
        }
        {
          T ar = cr[FB_OB + m], ai = ci[FB_OB + m];               // bin 2m + 1
          T br = cr[FB_OB + 63 - m], bi = -(T)ci[FB_OB + 63 - m]; // bin 127 - 2m
          rfft_unsplit(ar, ai, br, bi, wk1x, wk1y, s1r[u], s1i[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < NU; u++) { dit_stage<1, 5>(s0r[u], s0i[u], ltw); dit_stage<1, 5>(s1r[u], s1i[u], ltw); }
#pragma unroll
      for (int u = 0; u < NU; u++) { dit_stage<2, 4>(s0r[u], s0i[u], ltw); dit_stage<2, 4>(s1r[u], s1i[u], ltw); }
#pragma unroll
      for (int u = 0; u < NU; u++) { dit_stage<4, 3>(s0r[u], s0i[u], ltw); dit_stage<4, 3>(s1r[u], s1i[u], ltw); }
#pragma unroll
      for (int u = 0; u < NU; u++) { dit_stage<8, 2>(s0r[u], s0i[u], ltw); dit_stage<8, 2>(s1r[u], s1i[u], ltw); }
#pragma unroll
      for (int u = 0; u < NU; u++) { dit_stage<16, 1>(s0r[u], s0i[u], ltw); dit_stage<16, 1>(s1r[u], s1i[u], ltw); }
#pragma unroll
      for (int u = 0; u < NU; u++) { dit_stage<32, 0>(s0r[u], s0i[u], ltw); dit_stage<32, 0>(s1r[u], s1i[u], ltw); }
#pragma unroll
      for (int u = 0; u < NU; u++) {
        T qr = fma(s1r[u], ltw.c1, s1i[u] * ltw.s1), qi = fma(s1i[u], ltw.c1, -(s1r[u] * ltw.s1));
        const T scale = (T)(1.0 / 256.0);
        hd[bq][u][0] = (float)((s0r[u] + qr) * scale);   // time samples 2l, 2l+1
        hd[bq][u][1] = (float)((s0i[u] + qi) * scale);
        tl[bq][u][0] = (float)((s0r[u] - qr) * scale);   // time samples 128+2l, 128+2l+1
        tl[bq][u][1] = (float)((s0i[u] - qi) * scale);
      }
    }
  }
  GA_TL(3);
  __syncthreads();   // every wave is done reading the staging tile: reuse it as head[33][128] | tail[33][128]
  GA_TL(4);
  float* head = smem;
  float* tail = smem + 33 * kBlock;
#pragma unroll
  for (int bq = 0; bq < 3; bq++) {
    const int NU = bq < 2 ? 4 : 1;
    const bool mine = bq < 2 || wave == (int)(blockIdx.x & 3);
#pragma unroll
    for (int u = 0; u < NU; u++) {
      const int c = bq < 2 ? (bq * 4 + u) * 4 + wave : FB_RUN;
      if (mine && c <= nrun && (c > 0 || ta > 0)) {
        *reinterpret_cast<float2*>(&head[c * kBlock + 2 * lane]) = make_float2(hd[bq][u][0], hd[bq][u][1]);
        *reinterpret_cast<float2*>(&tail[c * kBlock + 2 * lane]) = make_float2(tl[bq][u][0], tl[bq][u][1]);
      }
    }
  }
  if (ta == 0 && tid < kBlock) tail[tid] = ldg1(overlap_in[row] + tid);   // incoming overlap of the chunk's first block
  __syncthreads();
  GA_TL(5);
  float* out = yrows[row].out;
  if (out) {
    float* o4 = out + (int64_t)ta * kBlock;
    for (int idx = tid; idx < nrun * (kBlock / 4); idx += 256) {
      const int c = idx / (kBlock / 4) + 1, s4 = (idx % (kBlock / 4)) * 4;
      const float4 h = *reinterpret_cast<const float4*>(&head[c * kBlock + s4]);
      const float4 t = *reinterpret_cast<const float4*>(&tail[(c - 1) * kBlock + s4]);
      stg4(o4 + 4 * idx, v4f{h.x + t.x, h.y + t.y, h.z + t.z, h.w + t.w});   // (float)y[i] + overlap[i]  (:148)
    }
  }
  if (tb == nblocks && tid < kBlock) stg1(overlap_out[row] + tid, tail[nrun * kBlock + tid]);   // overlap[i] = (float)y[i+128]  (:149)
  GA_TL(6);
}
void launch_irfft_ola_b(hipStream_t s, const ConvRowIO* yrows_dev, int ny, int nblocks, ConvPlanesB pl,
                        const float* const* overlap_in_dev, float* const* overlap_out_dev, Twiddles tw, bool fp64) {
  if (ny <= 0 || nblocks <= 0) return;
  for (int r0 = 0; r0 < ny; r0 += 65535) {   // gridDim.y limit
    dim3 grid((nblocks + FB_RUN - 1) / FB_RUN, std::min(65535, ny - r0));
    if (fp64) hipLaunchKernelGGL(irfft_ola_b_kernel<double>, grid, dim3(256), 0, s, yrows_dev, ny, nblocks, pl, overlap_in_dev, overlap_out_dev, tw, r0);
    else hipLaunchKernelGGL(irfft_ola_b_kernel<float>, grid, dim3(256), 0, s, yrows_dev, ny, nblocks, pl, overlap_in_dev, overlap_out_dev, tw, r0);
  }
}

}  // namespace ga
