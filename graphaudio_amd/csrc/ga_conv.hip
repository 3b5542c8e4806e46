// ga_conv.hip -- the fine-partition convolver outside formulation D: everything that prepares or applies an impulse response in
// 128-sample partitions (PartitionedConvolver.cs:104-223).  Formulation A (shared impulse response, spectral_mac_shared_kernel)
// and B (private impulse responses, spectral_mac_b_kernel) run the partition sum over ALL blocks of a render chunk at once: for
// one frequency bin it is a banded-Toeplitz GEMM  Y[rows x time] = X[rows x time'] * T(H)  on the f32 matrix cores
// (v_mfma_f32_16x16x4_f32, exact f32 fma chain), rows = convolver channel-instances sharing one IR channel.  Formulation R
// (refmac_kernel) is the same sum in the reference's own order; formulation C (tap_spectra_kernel, tconv_kernel, tconv16_kernel)
// is an FFT convolution along the block axis.  With them: the history copies (stale_copy_kernel, hist_copy_b_kernel), the plane
// utilities and the sample-rate converter of impulse responses (ir_resample_kernel, ga_ir_resample.hpp).  The 256-point transforms
// around the sums are in ga_rfft.hip.  Wave64, -ffp-contract=off: see ga_kernels.hip.

#include "ga_kernels.hpp"
#include "ga_device_common.hpp"
#include "ga_fft16.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace ga {

// =====================================================================================================
//  Shared-IR spectral multiply-accumulate on the f32 matrix cores.
//  Reference: PartitionedConvolver.ProcessSpectralConvolution, PartitionedConvolver.cs:154-223
//     acc[k] = sum_{p<P} FDL[(w+p)%P][k] * H[p][k]            (one block, one channel-instance)
//  Here, for one bin k and all blocks t of the chunk and all rows r sharing H:
//     Y[r][t] = sum_u X[r][t0 + u] * G[u - j],  j = t - t0,  G[m] = H[P-1-m] (0 <= m < P), a banded Toeplitz GEMM.
//  Workgroup tile 128 rows x 64 blocks; wave tile 32 rows x 64 blocks = 2 x 4 MFMA 16x16 tiles, re+im accumulators.
//  Taps are processed in segments of <= MAC_PSEG so the reversed taps fit LDS whatever P is.
// =====================================================================================================
constexpr int MAC_ROWS = 128;
constexpr int MAC_TIME = 64;
constexpr int MAC_KC = 16;                   // time steps (u) per LDS chunk
constexpr int MAC_LD = MAC_ROWS + 16;        // padded row stride: lanes 16..31 land 16 banks away from lanes 0..15
constexpr int MAC_PSEG = 1024;
constexpr int MAC_GLEN = MAC_PSEG + 160;

// One 16-step chunk of the banded Toeplitz product for a wave tile (2 M-tiles x 4 N-tiles).
// N-tile n (blocks 16n..16n+15 of the time tile) is inside the band exactly for chunks [n, n + (Ps+14)/16]: the band
// edges coincide with chunk boundaries, so activity is decided per (chunk, N-tile) with no wasted MFMA, and the partial
// edge chunks are covered by the zero padding of the reversed tap table.  A fragments are read once per chunk, B
// fragments are double buffered one N-tile ahead so their LDS latency hides under the previous tile's 24 MFMAs.
__device__ __forceinline__ void mac_chunk(const float* __restrict xsr, const float* __restrict xsi, const float* __restrict g0,
                                          const float* __restrict g1, const float* __restrict g2, int c, int Ps, int wave, int la,
                                          int lk, f32x4 (&acc1)[2][4], f32x4 (&acc2)[2][4], f32x4 (&acc3)[2][4]) {
  float ar[4][2], ai[4][2], as[4][2];
#pragma unroll
  for (int ks = 0; ks < 4; ks++)
#pragma unroll
    for (int m = 0; m < 2; m++) {
      int off = (ks * 4 + lk) * MAC_LD + wave * 32 + m * 16 + la;
      ar[ks][m] = xsr[off];
      ai[ks][m] = xsi[off];
    }
  float br[2][4], bi[2][4], bs[2][4];
  const int gbase = c * MAC_KC + lk - la + 64;
#pragma unroll
  for (int ks = 0; ks < 4; ks++) {
    br[0][ks] = g0[gbase + ks * 4];
    bi[0][ks] = g1[gbase + ks * 4];
    bs[0][ks] = g2[gbase + ks * 4];
  }
#pragma unroll
  for (int ks = 0; ks < 4; ks++)
#pragma unroll
    for (int m = 0; m < 2; m++) as[ks][m] = ar[ks][m] + ai[ks][m];
  const int last = (Ps + 14) / 16;
#pragma unroll
  for (int n = 0; n < 4; n++) {
    const int cur = n & 1, nxt = cur ^ 1;
    if (n + 1 < 4) {
#pragma unroll
      for (int ks = 0; ks < 4; ks++) {
        int gi = gbase + ks * 4 - 16 * (n + 1);
        br[nxt][ks] = g0[gi];
        bi[nxt][ks] = g1[gi];
        bs[nxt][ks] = g2[gi];
      }
    }
    if (c >= n && c <= n + last) {   // wave uniform
#pragma unroll
      for (int ks = 0; ks < 4; ks++)
#pragma unroll
        for (int m = 0; m < 2; m++) {
          // (a + ib)(c + id) = (ac - bd) + i(ad + bc)   (PartitionedConvolver.cs:195-204) on the matrix core
          acc1[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[ks][m], br[cur][ks], acc1[m][n], 0, 0, 0);
          acc2[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(ai[ks][m], bi[cur][ks], acc2[m][n], 0, 0, 0);
          acc3[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(as[ks][m], bs[cur][ks], acc3[m][n], 0, 0, 0);
        }
    }
  }
}

__global__ __launch_bounds__(256) void spectral_mac_shared_kernel(ConvPlanes pl, const float* __restrict hr, const float* __restrict hi,
                                                                 int P, int ntt, int nrt, int total) {
  __shared__ __attribute__((aligned(16))) float xs[2][2][MAC_KC * MAC_LD];   // [buffer][re/im][u][row]
  __shared__ float gs[3][MAC_GLEN];                                           // reversed, zero padded taps: re, im, re + im

  // XCD-aware mapping: workgroups b and b+8 share an XCD (round-robin dispatch), give each XCD a contiguous range of
  // (bin, row tile, time tile) so neighbouring time tiles -- which re-read 8/9 of the same X rows -- share one L2.
  const int per = (total + 7) >> 3;
  const int L = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
  if (L >= total) return;
  const int tt = L % ntt;
  const int rt = (L / ntt) % nrt;
  const int k = L / (ntt * nrt);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t0 = tt * MAC_TIME;
  const int row0 = rt * MAC_ROWS;
  const size_t xplane = (size_t)pl.tx * pl.rp;
  const float* __restrict xr = pl.xr + (size_t)k * xplane + row0;
  const float* __restrict xi = pl.xi + (size_t)k * xplane + row0;

  // Three-multiplication complex product (Gauss): with P1 = sum ar*br, P2 = sum ai*bi, P3 = sum (ar+ai)*(br+bi)
  //   re = P1 - P2 ,  im = P3 - P1 - P2      -> 3 MFMAs per complex tile step instead of 4.
  f32x4 acc1[2][4], acc2[2][4], acc3[2][4];
#pragma unroll
  for (int m = 0; m < 2; m++)
#pragma unroll
    for (int n = 0; n < 4; n++) {
      acc1[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
      acc2[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
      acc3[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }

  // global -> LDS staging is WAVE-PRIVATE: wave w only ever reads rows [32w, 32w+32) of a chunk, so it stages exactly
  // those rows itself (lane -> u = lane/8 and +8, rows 32w + 4*(lane%8) .. +3).  LDS operations of one wave execute in
  // order, so the main loop needs no workgroup barrier and the four waves drift freely over the shared matrix pipes.
  const int su = lane >> 3, sr4 = wave * 32 + (lane & 7) * 4;
  const int la = lane & 15, lk = lane >> 4;

  for (int pa = 0; pa < P; pa += MAC_PSEG) {
    const int Ps = min(MAC_PSEG, P - pa);
    const int u0 = P - (pa + Ps);                  // plane-row offset of this tap segment
    const int nch = (Ps + 63 + MAC_KC - 1) / MAC_KC + 0;
    __syncthreads();                               // previous segment's LDS fully consumed
    // G[m] for m in [-64, Ps+96): gs[m + 64]
    for (int i = tid; i < MAC_GLEN; i += 256) {
      int m = i - 64;
      bool ok = (m >= 0) && (m < Ps);
      int p = pa + Ps - 1 - m;
      float gr_ = ok ? hr[(size_t)k * P + p] : 0.f;
      float gi_ = ok ? hi[(size_t)k * P + p] : 0.f;
      gs[0][i] = gr_;
      gs[1][i] = gi_;
      gs[2][i] = gr_ + gi_;
    }
    // prologue: chunk 0
    float4 pr0, pr1, pi0, pi1;
    {
      size_t o0 = (size_t)(t0 + u0 + su) * pl.rp + sr4;
      size_t o1 = (size_t)(t0 + u0 + su + 8) * pl.rp + sr4;
      pr0 = *reinterpret_cast<const float4*>(xr + o0);
      pr1 = *reinterpret_cast<const float4*>(xr + o1);
      pi0 = *reinterpret_cast<const float4*>(xi + o0);
      pi1 = *reinterpret_cast<const float4*>(xi + o1);
    }
    *reinterpret_cast<float4*>(&xs[0][0][su * MAC_LD + sr4]) = pr0;
    *reinterpret_cast<float4*>(&xs[0][0][(su + 8) * MAC_LD + sr4]) = pr1;
    *reinterpret_cast<float4*>(&xs[0][1][su * MAC_LD + sr4]) = pi0;
    *reinterpret_cast<float4*>(&xs[0][1][(su + 8) * MAC_LD + sr4]) = pi1;
    __syncthreads();

    for (int c = 0; c < nch; c++) {
      const int buf = c & 1;
      const bool more = (c + 1) < nch;
      if (more) {
        size_t o0 = (size_t)(t0 + u0 + (c + 1) * MAC_KC + su) * pl.rp + sr4;
        size_t o1 = o0 + (size_t)8 * pl.rp;
        pr0 = *reinterpret_cast<const float4*>(xr + o0);
        pr1 = *reinterpret_cast<const float4*>(xr + o1);
        pi0 = *reinterpret_cast<const float4*>(xi + o0);
        pi1 = *reinterpret_cast<const float4*>(xi + o1);
      }
      mac_chunk(xs[buf][0], xs[buf][1], gs[0], gs[1], gs[2], c, Ps, wave, la, lk, acc1, acc2, acc3);
      if (more) {
        const int nb = buf ^ 1;
        *reinterpret_cast<float4*>(&xs[nb][0][su * MAC_LD + sr4]) = pr0;
        *reinterpret_cast<float4*>(&xs[nb][0][(su + 8) * MAC_LD + sr4]) = pr1;
        *reinterpret_cast<float4*>(&xs[nb][1][su * MAC_LD + sr4]) = pi0;
        *reinterpret_cast<float4*>(&xs[nb][1][(su + 8) * MAC_LD + sr4]) = pi1;
      }
      __builtin_amdgcn_wave_barrier();   // scheduling fence only: keep the staging writes ahead of the next chunk's reads
    }
  }

  // epilogue: C/D layout of v_mfma_f32_16x16x4_f32: column (time) = lane & 15, row = 4 * (lane >> 4) + reg
  const size_t yplane = (size_t)pl.ty * pl.rp;
  float* __restrict yr = pl.yr + (size_t)k * yplane + row0;
  float* __restrict yi = pl.yi + (size_t)k * yplane + row0;
#pragma unroll
  for (int m = 0; m < 2; m++)
#pragma unroll
    for (int n = 0; n < 4; n++) {
      int t = t0 + 16 * n + la;
      size_t o = (size_t)t * pl.rp + wave * 32 + m * 16 + lk * 4;
      *reinterpret_cast<f32x4*>(yr + o) = acc1[m][n] - acc2[m][n];
      *reinterpret_cast<f32x4*>(yi + o) = (acc3[m][n] - acc1[m][n]) - acc2[m][n];
    }
}

void launch_spectral_mac_shared(hipStream_t s, ConvPlanes pl, const float* hr, const float* hi, int P, int nblocks, int nrows) {
  if (nrows <= 0 || nblocks <= 0 || P <= 0) return;
  int ntt = (nblocks + MAC_TIME - 1) / MAC_TIME;
  int nrt = (nrows + MAC_ROWS - 1) / MAC_ROWS;
  int total = kBins * ntt * nrt;
  int grid = ((total + 7) / 8) * 8;
  hipLaunchKernelGGL(spectral_mac_shared_kernel, dim3(grid), dim3(256), 0, s, pl, hr, hi, P, ntt, nrt, total);
}

// MAC B: workgroup = (set, bin, 256-block time tile); wave = 64 blocks (4 M-tiles) x 16 columns; taps in segments of 256
constexpr int MB_TW = 256;
constexpr int MB_PSEG = 256;
constexpr int MB_HLD = MB_PSEG + 2;            // column stride: 2j + kk distinct banks for lanes (j, kk)
constexpr int MB_XLEN = MB_TW + MB_PSEG + 8;

__global__ __launch_bounds__(256) void spectral_mac_b_kernel(const ConvSetB* __restrict sets, int nblocks, int hist, ConvPlanesB pl,
                                                             int ntt) {
  __shared__ float hs[3][16 * MB_HLD];   // taps re, im, re+im  [column][p]
  __shared__ float xw[3][MB_XLEN];       // input spectra window re, im, re+im : xw[i] = X[t0 - pa - (Ps-1) + i ... ]
  const ConvSetB* __restrict Sp = &sets[blockIdx.z];   // accessed in place: a by-value copy (32 pointers) would go to scratch
  struct { int x, y0, ncol, P; } S = {Sp->x, Sp->y0, Sp->ncol, Sp->P};
  const int k = blockIdx.y;
  const int tt = blockIdx.x;
  const int t0 = tt * MB_TW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int la = lane & 15, lk = lane >> 4;
  const int P = S.P;
  const float* __restrict xr = pl.xr + ((size_t)S.x * kBins + k) * pl.tx;
  const float* __restrict xi = pl.xi + ((size_t)S.x * kBins + k) * pl.tx;

  f32x4 acc1[4], acc2[4], acc3[4];
#pragma unroll
  for (int m = 0; m < 4; m++) {
    acc1[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
    acc2[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
    acc3[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  for (int pa = 0; pa < P; pa += MB_PSEG) {
    const int Ps = min(MB_PSEG, P - pa);
    const int Ps4 = (Ps + 3) & ~3;
    __syncthreads();
    // taps of this segment, zero padded to a multiple of 4 (and unused columns zero)
    for (int i = tid; i < 16 * MB_HLD; i += 256) {
      int j = i / MB_HLD, p = i % MB_HLD;
      float vr = 0.f, vi = 0.f;
      if (j < S.ncol && p < Ps) {
        vr = Sp->hr[j][(size_t)k * P + pa + p];
        vi = Sp->hi[j][(size_t)k * P + pa + p];
      }
      hs[0][i] = vr;
      hs[1][i] = vi;
      hs[2][i] = vr + vi;
    }
    // window: plane index of block t is hist + t; tap p needs block t - p.  xw[i] <-> block  t0 - pa - (Ps4 - 1) + i
    const int wlen = MB_TW + Ps4 - 1;
    const int b0 = t0 - pa - (Ps4 - 1);
    for (int i = tid; i < wlen; i += 256) {
      int blk = b0 + i;            // may be < -hist (before any history): zero
      float vr = 0.f, vi = 0.f;
      if (blk >= -hist && blk < nblocks) {
        vr = xr[hist + blk];
        vi = xi[hist + blk];
      }
      xw[0][i] = vr;
      xw[1][i] = vi;
      xw[2][i] = vr + vi;
    }
    __syncthreads();
    // Y[t] += sum_p X[t - p] H[p];  A[i][kk] = X[t0w + 16m + i - (p0 + kk)] -> xw index (Ps4 - 1) + 64w + 16m + i - p0 - kk
    const int abase = (Ps4 - 1) + wave * 64 + la - lk;
    for (int p0 = 0; p0 < Ps4; p0 += 4) {
      const int hoff = la * MB_HLD + p0 + lk;
      float br = hs[0][hoff], bi = hs[1][hoff], bs = hs[2][hoff];
#pragma unroll
      for (int m = 0; m < 4; m++) {
        const int xo = abase + 16 * m - p0;
        float ar = xw[0][xo], ai = xw[1][xo], as = xw[2][xo];
        acc1[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar, br, acc1[m], 0, 0, 0);
        acc2[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(ai, bi, acc2[m], 0, 0, 0);
        acc3[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(as, bs, acc3[m], 0, 0, 0);
      }
    }
  }
  // D layout: column (IR channel) = lane & 15, row (block) = 4 * (lane >> 4) + reg -> four consecutive blocks per lane
  if (la < S.ncol) {
    float* __restrict yr = pl.yr + ((size_t)(S.y0 + la) * kBins + k) * pl.ty;
    float* __restrict yi = pl.yi + ((size_t)(S.y0 + la) * kBins + k) * pl.ty;
#pragma unroll
    for (int m = 0; m < 4; m++) {
      int t = t0 + wave * 64 + 16 * m + 4 * lk;
      if (t < pl.ty) {
        *reinterpret_cast<f32x4*>(yr + t) = acc1[m] - acc2[m];
        *reinterpret_cast<f32x4*>(yi + t) = (acc3[m] - acc1[m]) - acc2[m];
      }
    }
  }
}
void launch_spectral_mac_b(hipStream_t s, const ConvSetB* sets_dev, int nsets, int nblocks, int hist, ConvPlanesB pl) {
  if (nsets <= 0 || nblocks <= 0) return;
  int ntt = (nblocks + MB_TW - 1) / MB_TW;
  for (int z0 = 0; z0 < nsets; z0 += 32768) {   // gridDim.z limit
    int nz = std::min(32768, nsets - z0);
    hipLaunchKernelGGL(spectral_mac_b_kernel, dim3(ntt, kBins, nz), dim3(256), 0, s, sets_dev + z0, nblocks, hist, pl, ntt);
  }
}

// =====================================================================================================
//  Reference-order partition sum (formulation R): PartitionedConvolver.ProcessSpectralConvolution
//  (PartitionedConvolver.cs:154-223) evaluated EXACTLY as the reference evaluates it -- for every (row, block t, bin k)
//      acc = 0 ;  for p = 0 .. P-1:  acc.re += (X.re * H.re) - (X.im * H.im) ;  acc.im += (X.re * H.im) + (X.im * H.re)
//  with X = X[t - p][k], H = H[p][k], every operation a separately rounded float32 operation (the reference's AVX
//  Multiply / Subtract / Add and its scalar tail: no fused multiply-add anywhere) and the partitions in ascending order.
//  All (t, k) chains are independent: only the order INSIDE a chain is serial.  Around it run the double-precision
//  256-point transforms of the B layout (rfft_fwd_b_kernel<double> / irfft_ola_b_kernel<double>), so a convolver served by
//  this route reproduces the reference's float32 output bit for bit (up to the ~1e-9 chance per value that two correct
//  double-precision transforms round to different floats).  The planner takes it for convolvers whose output reaches
//  arithmetic that amplifies or quantises last-bit differences (Context::refOrderSensitivity).
//
//  Workgroup = (set, bin, tile of 1024 blocks), 4 waves; lane l of wave w owns the four consecutive blocks
//  t0 + 256 w + 4 l + {0..3}.  The window X[t0 - (Ps-1) .. t0 + 1023] of the bin and the taps H[p] sit in LDS as separate
//  re / im float arrays: per 4 taps a lane reads ONE aligned 16-byte quad of each (consecutive lanes: consecutive quads, no
//  bank conflict) and the taps by broadcast; the window slides through registers (two quads cover four taps x four blocks).  128 VALU operations per 4 LDS reads; taps beyond 1024 in further segments, accumulators carried.
// =====================================================================================================
constexpr int RM_TW = 1024;     // blocks per workgroup
constexpr int RM_PSEG = 1024;   // taps per segment

// Each operation is spelled out as one scalar VALU instruction: left to itself the compiler pairs the products and sums of
// neighbouring chains into v_pk_mul_f32 / v_pk_add_f32 and pays for the pairs with moves -- 58 v_mov per 68 packed operations in
// this loop, while a packed f32 instruction costs the same SIMD cycles as the two scalar ones it replaces on gfx950
// (profiles/r01_micro_pk_f32_issue_rate.txt).
#define GA_RM_OP(op, r, a, b) asm(op " %0, %1, %2" : "=v"(r) : "v"(a), "v"(b))
__device__ __forceinline__ void rm_cmac(float& ar, float& ai, float dr, float di, float hr, float hi) {
  // (dr * ir) - (di * ii) ; (dr * ii) + (di * ir) ; acc += ...   PartitionedConvolver.cs:196-206,218-219
  float p0, p1, p2, p3, re, im;
  GA_RM_OP("v_mul_f32", p0, dr, hr);
  GA_RM_OP("v_mul_f32", p1, di, hi);
  GA_RM_OP("v_mul_f32", p2, dr, hi);
  GA_RM_OP("v_mul_f32", p3, di, hr);
  GA_RM_OP("v_sub_f32", re, p0, p1);
  GA_RM_OP("v_add_f32", im, p2, p3);
  GA_RM_OP("v_add_f32", ar, ar, re);
  GA_RM_OP("v_add_f32", ai, ai, im);
}

__global__ __launch_bounds__(256) void refmac_kernel(const ConvSetB* __restrict sets, int nblocks, int hist, ConvPlanesB pl) {
  // w[i] <-> block  b0 + i ,  b0 = t0 - pa - (Ps4 - 1):  output block t0 + T + r needs, for tap pa + pp,  w[c + r - pp],  c = T + Ps4 - 1
  __shared__ __attribute__((aligned(16))) float wr[RM_TW + RM_PSEG + 4];
  __shared__ __attribute__((aligned(16))) float wi[RM_TW + RM_PSEG + 4];
  __shared__ __attribute__((aligned(16))) float hrs[RM_PSEG];
  __shared__ __attribute__((aligned(16))) float his[RM_PSEG];
  const ConvSetB* __restrict Sp = &sets[blockIdx.z];
  const int Sx = Sp->x, Sy0 = Sp->y0, ncol = Sp->ncol, P = Sp->P;
  const int k = blockIdx.y;
  const int t0 = blockIdx.x * RM_TW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = wave * 256 + 4 * lane;
  const GA_GLOBAL float* xr = gptr(pl.xr + ((size_t)Sx * kBins + k) * pl.tx);
  const GA_GLOBAL float* xi = gptr(pl.xi + ((size_t)Sx * kBins + k) * pl.tx);
  const bool oneSeg = P <= RM_PSEG;
  for (int j = 0; j < ncol; j++) {
    const GA_GLOBAL float* hr = gptr(Sp->hr[j] + (size_t)k * P);
    const GA_GLOBAL float* hi = gptr(Sp->hi[j] + (size_t)k * P);
    float ar[4] = {0.f, 0.f, 0.f, 0.f}, ai[4] = {0.f, 0.f, 0.f, 0.f};   // Array.Clear(_accReal / _accImag), :157-158
    for (int pa = 0; pa < P; pa += RM_PSEG) {
      const int Ps = min(RM_PSEG, P - pa);
      const int Ps4 = (Ps + 3) & ~3;   // (taps beyond Ps are zero: they add (+-)0 to the sums, which leaves every finite sum as it is)
      __syncthreads();
      for (int p = tid; p < Ps4; p += 256) {
        hrs[p] = p < Ps ? hr[pa + p] : 0.f;
        his[p] = p < Ps ? hi[pa + p] : 0.f;
      }
      if (!(oneSeg && j > 0)) {   // (one segment: the window is the same for every column)
        const int b0 = t0 - pa - (Ps4 - 1);
        const int wlen = RM_TW + Ps4 + 3;   // (+ 4: the unused tail of the newest quad)
        for (int i = tid; i < wlen; i += 256) {
          const int blk = b0 + i;   // plane index of block t is hist + t ; outside [-hist, nblocks): zero
          float vr = 0.f, vi = 0.f;
          if (blk >= -hist && blk < nblocks) {
            vr = xr[hist + blk];
            vi = xi[hist + blk];
          }
          wr[i] = vr;
          wi[i] = vi;
        }
      }
      __syncthreads();
      if (t0 + T < nblocks) {
        // quad Q_q = w[c - 4 q - 3 .. c - 4 q] (aligned: c == 3 mod 4).  Tap 4 q + s reads, for output r, w[c + r - 4 q - s]:
        //   s = 0: (Q_q.w, Q_{q-1}.x, .y, .z)   s = 1: (Q_q.z, Q_q.w, Q_{q-1}.x, .y)   s = 2: (Q_q.y, .z, .w, Q_{q-1}.x)   s = 3: Q_q
        int qi = T + Ps4;
        float4 pr = *reinterpret_cast<const float4*>(&wr[qi]);   // Q_{-1}: the three blocks behind the lane's first one
        float4 pi = *reinterpret_cast<const float4*>(&wi[qi]);
        for (int q = 0; q < Ps4; q += 4) {
          qi -= 4;
          const float4 cr = *reinterpret_cast<const float4*>(&wr[qi]);
          const float4 ci = *reinterpret_cast<const float4*>(&wi[qi]);
          const float4 gr = *reinterpret_cast<const float4*>(&hrs[q]);   // (broadcast reads)
          const float4 gi = *reinterpret_cast<const float4*>(&his[q]);
          rm_cmac(ar[0], ai[0], cr.w, ci.w, gr.x, gi.x);
          rm_cmac(ar[1], ai[1], pr.x, pi.x, gr.x, gi.x);
          rm_cmac(ar[2], ai[2], pr.y, pi.y, gr.x, gi.x);
          rm_cmac(ar[3], ai[3], pr.z, pi.z, gr.x, gi.x);
          rm_cmac(ar[0], ai[0], cr.z, ci.z, gr.y, gi.y);
          rm_cmac(ar[1], ai[1], cr.w, ci.w, gr.y, gi.y);
          rm_cmac(ar[2], ai[2], pr.x, pi.x, gr.y, gi.y);
          rm_cmac(ar[3], ai[3], pr.y, pi.y, gr.y, gi.y);
          rm_cmac(ar[0], ai[0], cr.y, ci.y, gr.z, gi.z);
          rm_cmac(ar[1], ai[1], cr.z, ci.z, gr.z, gi.z);
          rm_cmac(ar[2], ai[2], cr.w, ci.w, gr.z, gi.z);
          rm_cmac(ar[3], ai[3], pr.x, pi.x, gr.z, gi.z);
          rm_cmac(ar[0], ai[0], cr.x, ci.x, gr.w, gi.w);
          rm_cmac(ar[1], ai[1], cr.y, ci.y, gr.w, gi.w);
          rm_cmac(ar[2], ai[2], cr.z, ci.z, gr.w, gi.w);
          rm_cmac(ar[3], ai[3], cr.w, ci.w, gr.w, gi.w);
          pr = cr;
          pi = ci;
        }
      }
    }
    const int t = t0 + T;
    if (t < nblocks) {   // (t is a multiple of 4 and so is the planes' pitch: the quad stays inside the row)
      float* __restrict yr = pl.yr + ((size_t)(Sy0 + j) * kBins + k) * pl.ty;
      float* __restrict yi = pl.yi + ((size_t)(Sy0 + j) * kBins + k) * pl.ty;
      *reinterpret_cast<float4*>(yr + t) = make_float4(ar[0], ar[1], ar[2], ar[3]);
      *reinterpret_cast<float4*>(yi + t) = make_float4(ai[0], ai[1], ai[2], ai[3]);
    }
  }
}
void launch_refmac(hipStream_t s, const ConvSetB* sets_dev, int nsets, int nblocks, int hist, ConvPlanesB pl) {
  if (nsets <= 0 || nblocks <= 0) return;
  const int ntt = (nblocks + RM_TW - 1) / RM_TW;
  for (int z0 = 0; z0 < nsets; z0 += 32768) {   // gridDim.z limit
    const int nz = std::min(32768, nsets - z0);
    hipLaunchKernelGGL(refmac_kernel, dim3(ntt, kBins, nz), dim3(256), 0, s, sets_dev + z0, nblocks, hist, pl);
  }
}

__global__ __launch_bounds__(128) void stale_copy_kernel(const StaleJob* __restrict jobs) {
  const StaleJob j = jobs[blockIdx.x];
  const int i = threadIdx.x;
  gptr(j.dst)[i] = j.src ? ldg1(j.src + i) * (j.curve ? ldg1(j.curve + i) : j.scale) : 0.f;
}
void launch_stale_copy(hipStream_t s, const StaleJob* jobs_dev, int njobs) {
  if (njobs <= 0) return;
  hipLaunchKernelGGL(stale_copy_kernel, dim3(njobs), dim3(128), 0, s, jobs_dev);
}

// one wavefront per (job, bin): 4 bins per workgroup (a workgroup per bin moved 2 KB and was launch-rate bound)
__global__ __launch_bounds__(256) void hist_copy_b_kernel(const HistJobB* __restrict jobs) {
  const HistJobB j = jobs[blockIdx.y];
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= kBins) return;
  GA_GLOBAL float* __restrict d = gptr(j.dst) + (size_t)k * j.dst_stride;
  if (j.src) {
    const GA_GLOBAL float* __restrict sp = gptr(j.src) + (size_t)k * j.src_stride;
    for (int i = lane; i < j.n; i += 64) d[i] = sp[i];
  } else {
    for (int i = lane; i < j.n; i += 64) d[i] = 0.f;
  }
}
void launch_hist_copy_b(hipStream_t s, const HistJobB* jobs_dev, int njobs, int max_n) {
  if (njobs <= 0 || max_n <= 0) return;
  for (int j0 = 0; j0 < njobs; j0 += 32768) {
    int nj = std::min(32768, njobs - j0);
    hipLaunchKernelGGL(hist_copy_b_kernel, dim3((kBins + 3) / 4, nj), dim3(256), 0, s, jobs_dev + j0);
  }
}

// =====================================================================================================
//  Formulation C: FFT convolution along the block axis (see ga_kernels.hpp).  One workgroup of 256 threads owns one
//  N2-point complex sequence in LDS; Stockham autosort passes of radix 8 / 4 (natural order in and out), float32.
// =====================================================================================================
__device__ __forceinline__ float2 cmul(float2 a, float2 b) {   // explicit fma: 4 instructions, one rounding less per component
  return make_float2(fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x));
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cmul_mi(float2 a) { return make_float2(a.y, -a.x); }   // a * (-i)

__device__ __forceinline__ void dft4(float2& a0, float2& a1, float2& a2, float2& a3) {   // forward, natural order
  float2 t0 = cadd(a0, a2), t1 = csub(a0, a2), t2 = cadd(a1, a3), t3 = cmul_mi(csub(a1, a3));
  a0 = cadd(t0, t2);
  a2 = csub(t0, t2);
  a1 = cadd(t1, t3);
  a3 = csub(t1, t3);
}
__device__ __forceinline__ void dft8(float2 (&v)[8]) {   // forward 8-point DFT, natural order in / out
  const float h = 0.70710678118654752440f;
  float2 e0 = v[0], e1 = v[2], e2 = v[4], e3 = v[6];
  float2 o0 = v[1], o1 = v[3], o2 = v[5], o3 = v[7];
  dft4(e0, e1, e2, e3);
  dft4(o0, o1, o2, o3);
  // odd part times W8^q
  float2 w1 = make_float2(h * (o1.x + o1.y), h * (o1.y - o1.x));      // o1 * (1 - i)/sqrt2
  float2 w2 = cmul_mi(o2);                                            // o2 * (-i)
  float2 w3 = make_float2(h * (o3.y - o3.x), -h * (o3.x + o3.y));     // o3 * (-1 - i)/sqrt2
  v[0] = cadd(e0, o0); v[4] = csub(e0, o0);
  v[1] = cadd(e1, w1); v[5] = csub(e1, w1);
  v[2] = cadd(e2, w2); v[6] = csub(e2, w2);
  v[3] = cadd(e3, w3); v[7] = csub(e3, w3);
}

// LDS index padding: one extra float2 every 16 keeps the strided writes of the early passes off a single bank pair
__device__ __forceinline__ int PADI(int i) { return i + (i >> 4); }
#define TC_PADDED(n) ((n) + ((n) >> 4))

// one Stockham pass of radix R over the N-point sequence in `buf` (in place: read, barrier, write, barrier)
template <int N, int R>
__device__ __forceinline__ void stockham_pass(float2* __restrict buf, const float2* __restrict tw, int Ns, int tid) {
  constexpr int NB = N / R;                 // butterflies
  constexpr int PER = (NB + 255) / 256;     // per thread
  float2 v[PER][R];
#pragma unroll
  for (int u = 0; u < PER; u++) {
    const int j = tid + u * 256;
    if (NB % 256 == 0 || j < NB) {
      const int kk = j % Ns;
#pragma unroll
      for (int m = 0; m < R; m++) {
        float2 x = buf[PADI(j + m * NB)];
        if (m > 0) x = cmul(x, tw[(kk * m) * (N / (Ns * R))]);
        v[u][m] = x;
      }
      if constexpr (R == 8) {
        dft8(v[u]);
      } else {
        dft4(v[u][0], v[u][1], v[u][2], v[u][3]);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < PER; u++) {
    const int j = tid + u * 256;
    if (NB % 256 == 0 || j < NB) {
      const int kk = j % Ns;
      const int j0 = (j / Ns) * Ns * R + kk;
#pragma unroll
      for (int m = 0; m < R; m++) buf[PADI(j0 + m * Ns)] = v[u][m];
    }
  }
  __syncthreads();
}
template <int N>
__device__ __forceinline__ void fft_lds(float2* buf, const float2* tw, int tid) {   // forward N-point FFT in place
  if (N == 1024) {
    stockham_pass<N, 8>(buf, tw, 1, tid);
    stockham_pass<N, 8>(buf, tw, 8, tid);
    stockham_pass<N, 4>(buf, tw, 64, tid);
    stockham_pass<N, 4>(buf, tw, 256, tid);
  } else if (N == 2048) {
    stockham_pass<N, 8>(buf, tw, 1, tid);
    stockham_pass<N, 8>(buf, tw, 8, tid);
    stockham_pass<N, 8>(buf, tw, 64, tid);
    stockham_pass<N, 4>(buf, tw, 512, tid);
  } else {
    stockham_pass<N, 8>(buf, tw, 1, tid);
    stockham_pass<N, 8>(buf, tw, 8, tid);
    stockham_pass<N, 8>(buf, tw, 64, tid);
    stockham_pass<N, 8>(buf, tw, 512, tid);
  }
}

template <int N2>
__global__ __launch_bounds__(256) void tap_spectra_kernel(float2* __restrict hs, const float* __restrict hr, const float* __restrict hi,
                                                          int P, const float2* __restrict tw) {
  __shared__ float2 buf[TC_PADDED(N2)];
  const int k = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
  const size_t src = ((size_t)c * kBins + k) * P;
  for (int i = tid; i < N2; i += 256) buf[PADI(i)] = i < P ? make_float2(hr[src + i], hi[src + i]) : make_float2(0.f, 0.f);
  __syncthreads();
  fft_lds<N2>(buf, tw, tid);
  float2* dst = hs + ((size_t)c * kBins + k) * N2;
  // stored with the 1/N2 of the inverse transform folded in (a power of two: exact)
  const float sc = 1.0f / N2;
  for (int i = tid; i < N2; i += 256) dst[i] = make_float2(buf[PADI(i)].x * sc, buf[PADI(i)].y * sc);
}
const char* launch_tap_spectra(hipStream_t s, float2* hs, const float* hr, const float* hi, int nch, int P, int N2, const float2* tw) {
  dim3 g(kBins, nch), b(256);
  if (N2 == 1024) { hipLaunchKernelGGL(tap_spectra_kernel<1024>, g, b, 0, s, hs, hr, hi, P, tw); return "tap_spectra_kernel<1024>"; }
  if (N2 == 2048) { hipLaunchKernelGGL(tap_spectra_kernel<2048>, g, b, 0, s, hs, hr, hi, P, tw); return "tap_spectra_kernel<2048>"; }
  if (N2 == 4096) { hipLaunchKernelGGL(tap_spectra_kernel<4096>, g, b, 0, s, hs, hr, hi, P, tw); return "tap_spectra_kernel<4096>"; }
  launch_fail("no taps-spectrum kernel for this block-axis FFT length");
}

// ---- register/LDS hybrid FFT for the tconv kernel -------------------------------------------------------------------
// Every thread owns the PT = N/256 points {tid + 256 m}.  With the radix plans below these are exactly the inputs of the
// FIRST Stockham pass (butterfly j = tid + 256u reads j + (N/R1) m) and the outputs of the LAST one (j + (N/RL) m), so
// a forward FFT, a pointwise product and an inverse FFT chain through registers; only the middle passes go through LDS
// (ping-pong buffers, one barrier per pass).   N = 1024: radices 4,8,8,4   N = 2048: 8,8,8,4   N = 4096: 8,8,8,8
template <int R>
__device__ __forceinline__ void dftR(float2 (&v)[R]) {
  if constexpr (R == 8) dft8(v);
  else dft4(v[0], v[1], v[2], v[3]);
}
template <int N, int R>
__device__ __forceinline__ void first_pass(const float2 (&own)[N / 256], float2* __restrict dst, int tid) {
  constexpr int NBT = (N / R) / 256;   // butterflies per thread
#pragma unroll
  for (int u = 0; u < NBT; u++) {
    const int j = tid + 256 * u;
    float2 v[R];
#pragma unroll
    for (int m = 0; m < R; m++) v[m] = own[u + NBT * m];
    dftR<R>(v);
#pragma unroll
    for (int m = 0; m < R; m++) dst[PADI(j * R + m)] = v[m];   // Ns = 1: j0 = j * R
  }
}
template <int N, int R, int Ns>
__device__ __forceinline__ void mid_pass(const float2* __restrict src, float2* __restrict dst, const float2* __restrict tw, int tid) {
  constexpr int NB = N / R;
  constexpr int PER = (NB + 255) / 256;
#pragma unroll
  for (int u = 0; u < PER; u++) {
    const int j = tid + 256 * u;
    if (NB % 256 == 0 || j < NB) {
      const int kk = j % Ns;
      float2 v[R];
#pragma unroll
      for (int m = 0; m < R; m++) {
        float2 x = src[PADI(j + m * NB)];
        if (m > 0) x = cmul(x, tw[PADI((kk * m) * (N / (Ns * R)))]);
        v[m] = x;
      }
      dftR<R>(v);
      const int j0 = (j / Ns) * Ns * R + kk;
#pragma unroll
      for (int m = 0; m < R; m++) dst[PADI(j0 + m * Ns)] = v[m];
    }
  }
}
template <int N, int R>
__device__ __forceinline__ void last_pass(const float2* __restrict src, float2 (&own)[N / 256], const float2* __restrict tw, int tid) {
  constexpr int NB = N / R, Ns = N / R;   // last pass: Ns * R == N
  constexpr int NBT = NB / 256;
#pragma unroll
  for (int u = 0; u < NBT; u++) {
    const int j = tid + 256 * u;           // j < Ns: kk = j, j0 = j
    float2 v[R];
#pragma unroll
    for (int m = 0; m < R; m++) {
      float2 x = src[PADI(j + m * NB)];
      if (m > 0) x = cmul(x, tw[PADI(j * m)]);
      v[m] = x;
    }
    dftR<R>(v);
#pragma unroll
    for (int m = 0; m < R; m++) own[u + (Ns / 256) * m] = v[m];   // position j + m * Ns = tid + 256 (u + (Ns/256) m)
  }
}
// forward FFT of the thread-owned points; `a` is written first.  One barrier per pass.
template <int N>
__device__ __forceinline__ void fft_own(float2 (&own)[N / 256], float2* a, float2* b, const float2* tw, int tid) {
  if constexpr (N == 1024) {
    first_pass<N, 4>(own, a, tid);
    __syncthreads();
    mid_pass<N, 8, 4>(a, b, tw, tid);
    __syncthreads();
    mid_pass<N, 8, 32>(b, a, tw, tid);
    __syncthreads();
    last_pass<N, 4>(a, own, tw, tid);
  } else if constexpr (N == 2048) {
    first_pass<N, 8>(own, a, tid);
    __syncthreads();
    mid_pass<N, 8, 8>(a, b, tw, tid);
    __syncthreads();
    mid_pass<N, 8, 64>(b, a, tw, tid);
    __syncthreads();
    last_pass<N, 4>(a, own, tw, tid);
  } else {
    first_pass<N, 8>(own, a, tid);
    __syncthreads();
    mid_pass<N, 8, 8>(a, b, tw, tid);
    __syncthreads();
    mid_pass<N, 8, 64>(b, a, tw, tid);
    __syncthreads();
    last_pass<N, 8>(a, own, tw, tid);
  }
}

// Persistent workgroups: grid = (TC_GROUPS, bins).  A workgroup owns one bin and walks over its share of the
// (set, overlap-save segment) items: window of N2 block-spectra of the x-row -> FFT -> per column: * taps spectrum, inverse
// FFT (conjugation trick), store the N2 - P + 1 valid blocks of the y-row.  The twiddle table is brought into LDS once
// per workgroup, the bin's taps spectra stay in L2 (every concurrently running workgroup of the bin reads the same ones),
// and the NEXT item's window is prefetched into registers while the current item is transformed.
constexpr int TC_GROUPS = 17;   // 17 x 129 workgroups = 2.9 rounds of the 768 resident slots (3 per CU)
template <int N2>
__global__ __launch_bounds__(256) void tconv_kernel(const ConvSetC* __restrict sets, int nsets, int nseg, int nblocks, int hist,
                                                    ConvPlanesB pl, const float2* __restrict twg) {
  constexpr int PT = N2 / 256;
  extern __shared__ float2 lds[];
  float2* bufA = lds;
  float2* bufB = lds + TC_PADDED(N2);
  float2* tw = lds + 2 * TC_PADDED(N2);      // twiddle table exp(-2 pi i j / N2) in LDS
  const int k = blockIdx.y, tid = threadIdx.x;
  const int total = nsets * nseg;
  for (int i = tid; i < N2; i += 256) tw[PADI(i)] = twg[i];

  auto load_window = [&](int item, float2 (&w)[PT]) {
    const ConvSetC* __restrict S = &sets[item / nseg];
    const int seg = item % nseg;
    const int P = S->P;
    const int b0 = seg * (N2 - (P - 1)) - (P - 1);     // block of window element 0
    const float* __restrict xr = pl.xr + ((size_t)S->x * kBins + k) * pl.tx;
    const float* __restrict xi = pl.xi + ((size_t)S->x * kBins + k) * pl.tx;
#pragma unroll
    for (int m = 0; m < PT; m++) {
      const int blk = b0 + tid + 256 * m;
      w[m] = make_float2(0.f, 0.f);
      if (blk >= -hist && blk < nblocks) w[m] = make_float2(xr[hist + blk], xi[hist + blk]);
    }
  };

  int item = blockIdx.x;
  __syncthreads();                             // twiddles visible
  int flip = 0;
  while (item < total) {
    const ConvSetC* __restrict S = &sets[item / nseg];
    const int seg = item % nseg;
    const int P = S->P, ncol = S->ncol;
    const int L = N2 - (P - 1);
    const int t0 = seg * L;                    // first output block of this segment
    float2 xf[PT];
    load_window(item, xf);
    const int next = item + gridDim.x;
    if (t0 < nblocks) {
      // buffers alternate between consecutive transforms so that a fast thread never overwrites what a slower one still reads
      if (flip) fft_own<N2>(xf, bufB, bufA, tw, tid); else fft_own<N2>(xf, bufA, bufB, tw, tid);
      flip ^= 1;
      const float scale = 1.0f;   // 1/N2 is folded into the taps spectra (tap_spectra_kernel)
      const int nvalid = min(L, nblocks - t0);
      for (int j = 0; j < ncol; j++) {
        const float2* __restrict hs = S->hs[j] + (size_t)k * N2;
        float2 y[PT];
#pragma unroll
        for (int m = 0; m < PT; m++) {
          float2 p = cmul(xf[m], hs[tid + 256 * m]);
          y[m] = make_float2(p.x, -p.y);       // conj: ifft(v) = conj(fft(conj(v))) / N
        }
        if (flip) fft_own<N2>(y, bufB, bufA, tw, tid); else fft_own<N2>(y, bufA, bufB, tw, tid);
        flip ^= 1;
        float* __restrict yr = pl.yr + ((size_t)(S->y0 + j) * kBins + k) * pl.ty + t0;
        float* __restrict yi = pl.yi + ((size_t)(S->y0 + j) * kBins + k) * pl.ty + t0;
#pragma unroll
        for (int m = 0; m < PT; m++) {
          const int i = tid + 256 * m - (P - 1);   // output block index within the segment
          if (i >= 0 && i < nvalid) {
            yr[i] = y[m].x * scale;
            yi[i] = -y[m].y * scale;
          }
        }
      }
    }
    item = next;
  }
}
const char* launch_tconv(hipStream_t s, const ConvSetC* sets_dev, int nsets, int nblocks, int hist, ConvPlanesB pl, int N2, const float2* tw,
                         int nseg) {
  if (nsets <= 0 || nblocks <= 0) return "";
  size_t lds = ((size_t)3 * TC_PADDED(N2)) * sizeof(float2);
  // N2 = 4096 needs 104 KB of dynamic LDS (gfx950 has 160 KB per CU); per device, so set on every launch of this legacy path
  if (N2 == 4096) (void)hipFuncSetAttribute((const void*)tconv_kernel<4096>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096);
  // every set of one launch has the same P, hence the same segment length L = N2 - P + 1
  const long long total = (long long)nsets * nseg;
  const int gx = (int)std::min<long long>(total, TC_GROUPS);
  dim3 grid(gx, kBins), block(256);
  if (N2 == 1024) { hipLaunchKernelGGL(tconv_kernel<1024>, grid, block, lds, s, sets_dev, nsets, nseg, nblocks, hist, pl, tw); return "tconv_kernel<1024>"; }
  if (N2 == 2048) { hipLaunchKernelGGL(tconv_kernel<2048>, grid, block, lds, s, sets_dev, nsets, nseg, nblocks, hist, pl, tw); return "tconv_kernel<2048>"; }
  if (N2 == 4096) { hipLaunchKernelGGL(tconv_kernel<4096>, grid, block, lds, s, sets_dev, nsets, nseg, nblocks, hist, pl, tw); return "tconv_kernel<4096>"; }
  launch_fail("no block-axis FFT kernel for this length");
}

// (packed-f32 complex arithmetic and the radix-16 register / LDS transform live in ga_fft16.hpp)
// Persistent workgroups (one per resident slot).  The G transforms of a workgroup serve G different (set, segment) items.
template <int N2>
__global__ __launch_bounds__(256, 3) void tconv16_kernel(const ConvSetC* __restrict sets, int nsets, int nseg, int nblocks, int hist,
                                                      ConvPlanesB pl, const float2* __restrict twg, int tbase) {
  using PL = R16Plan<N2>;
  constexpr int T = PL::T, G = PL::G;
  extern __shared__ f2 lds16[];
  f2* lds = lds16;
  f2* tw2 = lds;
  f2* tw3 = lds + PL::T2;
  const int tid = threadIdx.x;
  // T >= 64: a wavefront belongs to ONE transform, so everything indexed by g is wave-uniform -- say so (scalar loads of
  // the set record, SGPR base addresses for the global accesses)
  const int g = __builtin_amdgcn_readfirstlane(tid / T), t = tid % T;
  f2* buf = lds + PL::T2 + PL::T3 + g * TC16_PADDED(N2);
  for (int i = tid; i < PL::T2 + PL::T3; i += 256) lds[i] = f2{twg[i].x, twg[i].y};
  const int total = nsets * nseg;
  __syncthreads();
  // work unit = (bin, step of G items); the units are dealt to the resident workgroups in contiguous, equal ranges (bin-major:
  // a workgroup stays on one bin, whose taps spectra stay in its L2)
  const int steps = (total + G - 1) / G;
  const long long units = (long long)kBins * steps;
  const long long per = (units + gridDim.x - 1) / gridDim.x;
  const long long w0 = (long long)blockIdx.x * per, w1 = min(units, w0 + per);
  const unsigned ut = (unsigned)t;
  // window of unit w -> registers.  Called for unit w + 1 as soon as the last product of unit w has consumed the spectrum,
  // so the HBM latency of the next window hides behind the last inverse transform.
  auto load_window = [&](long long w, f2 (&xw)[16]) {
    const int k = (int)(w / steps);
    const int item = (int)(w % steps) * G + g;
    const bool live = item < total;
    const ConvSetC* __restrict S = &sets[live ? item / nseg : 0];
    const int seg = live ? item % nseg : 0;
    const int P = S->P;
    const int t0 = tbase + seg * (N2 - (P - 1));
    // window element e = t + T m is block t0 - (P - 1) + e; plane index hist + block >= 0 because hist >= P - 1 (tconv16_hist_ok)
    const int first = hist + t0 - (P - 1);
    const int lim = (live && t0 < nblocks) ? nblocks - (t0 - (P - 1)) : 0;   // elements at or beyond `lim` are zero padding
    const float* __restrict xr = pl.xr + ((size_t)S->x * kBins + k) * pl.tx + first;
    const float* __restrict xi = pl.xi + ((size_t)S->x * kBins + k) * pl.tx + first;
#pragma unroll
    for (int m = 0; m < 16; m++) {
      xw[m] = f2{0.f, 0.f};
      if ((int)(ut + T * m) < lim) xw[m] = f2{xr[ut + T * m], xi[ut + T * m]};
    }
  };
  f2 xf[16];
  if (w0 < w1) load_window(w0, xf);
  for (long long w = w0; w < w1; w++) {
    const int k = (int)(w / steps);
    const int base = (int)(w % steps) * G;
    const int item = base + g;
    const bool live = item < total;
    const ConvSetC* __restrict S = &sets[live ? item / nseg : 0];
    const int seg = live ? item % nseg : 0;
    const int P = S->P;
    const int ncol = live ? S->ncol : 0;
    const int L = N2 - (P - 1);
    const int t0 = tbase + seg * L;
    const bool work = live && t0 < nblocks;
    int maxcol = 0;   // the same for every thread of the workgroup: barriers inside fft16_own
#pragma unroll
    for (int gg = 0; gg < G; gg++) {
      const int it = base + gg;
      if (it < total && tbase + (it % nseg) * L < nblocks) maxcol = max(maxcol, sets[it / nseg].ncol);
    }
    if (maxcol == 0) {
      if (w + 1 < w1) load_window(w + 1, xf);
      continue;
    }
    fft16_own<N2>(xf, buf, tw2, tw3, t);
    __syncthreads();   // the last-pass reads are done before the next transform stores into the buffer
    const int nvalid = min(L, nblocks - t0);
    for (int j = 0; j < maxcol; j++) {
      const bool act = work && j < ncol;
      f2 y[16];
      if (act) {
        const GA_GLOBAL f2* __restrict hs = reinterpret_cast<const GA_GLOBAL f2*>(gptr(S->hs[j]) + (size_t)k * N2);
#pragma unroll
        for (int m = 0; m < 16; m++) y[m] = cmulp_swap(xf[m], hs[ut + T * m]);   // ifft(v) = swap(fft(swap(v))) / N, 1/N inside hs
      } else {
#pragma unroll
        for (int m = 0; m < 16; m++) y[m] = f2{0.f, 0.f};
      }
      if (j == maxcol - 1 && w + 1 < w1) load_window(w + 1, xf);
      fft16_own<N2>(y, buf, tw2, tw3, t);
      if (act) {
        // element e = t + T m of the result is output block t0 + e - (P - 1); valid for P - 1 <= e < P - 1 + nvalid
        float* __restrict yr = pl.yr + ((size_t)(S->y0 + j) * kBins + k) * pl.ty + t0 - (P - 1);
        float* __restrict yi = pl.yi + ((size_t)(S->y0 + j) * kBins + k) * pl.ty + t0 - (P - 1);
        const int e0 = P - 1, e1 = P - 1 + nvalid;
#pragma unroll
        for (int m = 0; m < 16; m++) {
          const int e = (int)(ut + T * m);
          if (e >= e0 && e < e1) {
            yr[ut + T * m] = y[m].y;   // swapped back
            yi[ut + T * m] = y[m].x;
          }
        }
      }
      __syncthreads();
    }
  }
}
template <int N2>
static void launch_tconv16_n(hipStream_t s, const ConvSetC* sets_dev, int nsets, int nblocks, int hist, ConvPlanesB pl, const float2* tw16,
                             int nseg, int tbase) {
  using PL = R16Plan<N2>;
  const size_t lds = (size_t)(PL::T2 + PL::T3 + PL::G * TC16_PADDED(N2)) * sizeof(float2);
  // resident workgroups per device (a process may drive several devices: the attribute and the occupancy are per device)
  static int groupsOf[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) launch_fail("device ordinal out of range");
  if (!groupsOf[dev]) {
    if (hipFuncSetAttribute((const void*)tconv16_kernel<N2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096) != hipSuccess)
      launch_fail("cannot raise the dynamic LDS limit of the block-axis FFT kernel");
    int occ = 0, cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, tconv16_kernel<N2>, 256, lds) != hipSuccess || occ < 1)
      launch_fail("block-axis FFT kernel does not fit a compute unit");
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    groupsOf[dev] = occ * cus;   // exactly one resident round
  }
  const int groups = groupsOf[dev];
  const long long steps = ((long long)nsets * nseg + PL::G - 1) / PL::G;
  dim3 grid((unsigned)std::min<long long>(steps * kBins, groups)), block(256);
  hipLaunchKernelGGL(tconv16_kernel<N2>, grid, block, lds, s, sets_dev, nsets, nseg, nblocks, hist, pl, tw16, tbase);
}
const char* launch_tconv16(hipStream_t s, const ConvSetC* sets_dev, int nsets, int nblocks, int hist, ConvPlanesB pl, int N2, const float2* tw16,
                           int nseg, int tbase) {
  if (nsets <= 0 || nblocks <= 0 || nseg <= 0) return "";
  if (N2 == 1024) { launch_tconv16_n<1024>(s, sets_dev, nsets, nblocks, hist, pl, tw16, nseg, tbase); return "tconv16_kernel<1024>"; }
  if (N2 == 2048) { launch_tconv16_n<2048>(s, sets_dev, nsets, nblocks, hist, pl, tw16, nseg, tbase); return "tconv16_kernel<2048>"; }
  if (N2 == 4096) { launch_tconv16_n<4096>(s, sets_dev, nsets, nblocks, hist, pl, tw16, nseg, tbase); return "tconv16_kernel<4096>"; }
  launch_fail("no block-axis FFT kernel for this length");
}

// ---- plane utilities ----------------------------------------------------------------------------------
__global__ void plane_copy_kernel(float* __restrict dst, int dst_t, int dst_t0, const float* __restrict src, int src_t, int src_t0,
                                  int n, int rp) {
  const int k = blockIdx.y;
  const size_t per = (size_t)n * rp / 4;
  float4* d = reinterpret_cast<float4*>(dst + ((size_t)k * dst_t + dst_t0) * rp);
  const float4* s = src ? reinterpret_cast<const float4*>(src + ((size_t)k * src_t + src_t0) * rp) : nullptr;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < per; i += (size_t)gridDim.x * blockDim.x)
    d[i] = s ? s[i] : make_float4(0.f, 0.f, 0.f, 0.f);
}
void launch_plane_copy(hipStream_t s, float* dst, int dst_t, int dst_t0, const float* src, int src_t, int src_t0, int n, int rp) {
  if (n <= 0) return;
  size_t per = (size_t)n * rp / 4;
  int gx = (int)((per + 255) / 256);
  if (gx > 512) gx = 512;
  hipLaunchKernelGGL(plane_copy_kernel, dim3(gx, kBins), dim3(256), 0, s, dst, dst_t, dst_t0, src, src_t, src_t0, n, rp);
}

__global__ void extract_ir_kernel(float* __restrict hr, float* __restrict hi, const float* __restrict xr, const float* __restrict xi,
                                  int tx, int rp, int P, int nch) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;   // over nch * kBins * P
  int total = nch * kBins * P;
  if (idx >= total) return;
  int p = idx % P, k = (idx / P) % kBins, c = idx / (P * kBins);
  size_t o = ((size_t)k * tx + p) * rp + c;
  hr[idx] = xr[o];
  hi[idx] = xi[o];
}
void launch_extract_ir(hipStream_t s, float* hr, float* hi, const float* xr, const float* xi, int tx, int rp, int P, int nch) {
  int total = nch * kBins * P;
  if (total <= 0) return;
  hipLaunchKernelGGL(extract_ir_kernel, dim3((total + 255) / 256), dim3(256), 0, s, hr, hi, xr, xi, tx, rp, P, nch);
}

__global__ void pair_sum_kernel(float* __restrict out, const float* __restrict a, const float* __restrict b, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = a[i] + b[i];
}
void launch_pair_sum(hipStream_t s, float* out, const float* a, const float* b, int64_t n) {
  if (n <= 0) return;
  int g = (int)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(pair_sum_kernel, dim3(g), dim3(256), 0, s, out, a, b, n);
}

// ======================================================================================================
//  Sample-rate conversion of an impulse response / HRIR set (ga_ir_resample.hpp): workgroup = (tile of outputs, channel), lane =
//  output.  The tile's input window x[q_first - W + 1 .. q_last + W], clipped to the row, is staged once in LDS; every lane then walks
//  its output's 2W terms through ga_irr::ir_resample_sample -- the function the host calls -- so the sums are the same operations on
//  the same numbers.  Neighbouring lanes read the window D / L frames apart: for a ratio such as 24 (192 -> 8 kHz) that is 8 lanes
//  on one bank of the 32 a ds_read_b32 sees, so the LDS image skips one dword after every 32 (frame i at i + i / 32), which leaves
//  at most 2.  The table row of a lane (r = m D mod L) is read from global memory: L x 2W doubles stay cache resident (176 KB at
//  44.1 -> 48 kHz).  Runs once per buffer: milliseconds for a million taps, nothing here is tuned further.
// ======================================================================================================
constexpr int kIrResampleLds = kIrResampleWindow + kIrResampleWindow / 32 + 8;   // 8192 floats
static_assert(kIrResampleLds * sizeof(float) <= 32 * 1024, "the window's LDS image stays within 32 KB");
__device__ __forceinline__ int ir_resample_slot(int i) { return i + (i >> 5); }
__global__ __launch_bounds__(256) void ir_resample_kernel(const float* __restrict x, int64_t xstride, int64_t N, float* __restrict y, int64_t ystride,
                                                          int64_t M, int64_t L, int64_t D, int W, int tile, double gain, const double* __restrict tab) {
  __shared__ float win[kIrResampleLds];
  const int64_t m0 = (int64_t)blockIdx.x * tile;
  if (m0 >= M) return;
  const int64_t m1 = m0 + tile < M ? m0 + tile : M;
  const int64_t qa = m0 * D / L, qb = (m1 - 1) * D / L;
  const int64_t klo = qa - W + 1 > 0 ? qa - W + 1 : 0;
  const int64_t khi = qb + W + 1 < N ? qb + W + 1 : N;
  const int64_t wlen = khi - klo;
  if (wlen < 0 || wlen > kIrResampleWindow) return;   // (launch_ir_resample sized the tile so that this cannot happen)
  const GA_GLOBAL float* __restrict row = gptr(x) + (int64_t)blockIdx.y * xstride + klo;
  for (int i = threadIdx.x; i < (int)wlen; i += 256) win[ir_resample_slot(i)] = row[i];
  __syncthreads();
  const int64_t m = m0 + threadIdx.x;
  if (m >= m1) return;
  const int64_t q = m * D / L, r = m * D - q * L;
  const float* w = win;
  gptr(y)[(int64_t)blockIdx.y * ystride + m] =
      ga_irr::ir_resample_sample([w, klo](int64_t k) { return w[ir_resample_slot((int)(k - klo))]; }, q, N, W, tab + r * 2 * W, gain);
}
int ir_resample_tile(int64_t L, int64_t D, int W) {
  if (L < 1 || D < 1 || W < 1) return 0;
  const int64_t room = (int64_t)kIrResampleWindow - 2 * (int64_t)W - 1;   // frames q_last may lie behind q_first
  if (room < 0) return 0;
  // q(m0 + T - 1) - q(m0) <= floor((T - 1) D / L) + 1
  const int64_t t = room > ((int64_t)1 << 40) / L ? 256 : room * L / D + 1;
  return (int)(t < 256 ? t : 256);
}
void launch_ir_resample(hipStream_t s, const float* x, int64_t xstride, int64_t N, float* y, int64_t ystride, int64_t M, int channels,
                        int64_t L, int64_t D, int W, double gain, const double* tab_dev, int64_t tab_entries) {
  constexpr int64_t kBig = (int64_t)1 << 61;
  if (!x || !y || !tab_dev) launch_fail("ir_resample_kernel: null pointer");
  if (channels < 1 || channels > 65535) launch_fail("ir_resample_kernel: channels");
  if (L < 1 || D < 1 || W < 1 || L > ga_irr::kMaxTable || D > ((int64_t)1 << 31) || tab_entries != L * 2 * (int64_t)W || tab_entries > ga_irr::kMaxTable)
    launch_fail("ir_resample_kernel: plan");
  if (N < 1 || N > kBig / L || N > kBig / D) launch_fail("ir_resample_kernel: input length");
  if (M != ga_irr::ir_resample_length(N, L, D) || M < 1 || M > kBig / D) launch_fail("ir_resample_kernel: output length");
  if (xstride < N || ystride < M) launch_fail("ir_resample_kernel: stride");
  const int tile = ir_resample_tile(L, D, W);
  if (tile < 1) launch_fail("ir_resample_kernel: the window of one output does not fit");
  const int64_t tiles = (M + tile - 1) / tile;
  if (tiles > 0x7fffffff) launch_fail("ir_resample_kernel: too many tiles");
  hipLaunchKernelGGL(ir_resample_kernel, dim3((unsigned)tiles, (unsigned)channels), dim3(256), 0, s, x, xstride, N, y, ystride, M, L, D, W, tile, gain, tab_dev);
}

}  // namespace ga
