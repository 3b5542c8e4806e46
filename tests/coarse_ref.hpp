// coarse_ref.hpp -- a plain float64 statement of what the kernels of graphaudio_amd/csrc/ga_coarse.hip (formulation D of the convolver)
// compute, written from the contracts in ga_kernels.hpp and the comments of ga_coarse.hip, not from the kernels' index arithmetic.
// C++17, no HIP, nothing from csrc but the two constants restated below (tests/coarse_kernels_main.hip asserts they agree).
// Used by tests/coarse_ref_main.cpp (the reference against itself, under the sanitizers) and tests/coarse_kernels_main.hip (the
// kernels against the reference).
//
// Scale factors, as ga_engine.cpp states them at ensureCoarseSpectra: the forward kernel leaves out the 1/2 of its even/odd split, so
// a frame holds TWICE the spectrum (times the row's `scale`); the inverse kernel leaves out the 1/4 of its two splits and the 1/4096
// of its complex transforms, so it returns the UNNORMALISED inverse sum  x[n] = sum_k Y[k] e^(+2 pi i k n / N)  -- 16384 times the
// inverse transform.  With impulse responses transformed at scale 2^-16 the chain is 2 x 2 x 2^-16 x 2^14 = 1.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace coarse_ref {

constexpr int CB = 8192;     // kCoarseBlock: samples per coarse partition / output block
constexpr int NB = 8192;     // kCoarseBins: packed complex values of one 16,384-point real spectrum
constexpr int N = 2 * CB;    // points of a window

template <class T>
struct Cx {
  T re, im;
};
using cd = Cx<double>;

// in-place radix-2 decimation-in-time transform of n = 2^k points (twiddles computed in double and rounded to T once); sign = -1:
// forward, +1: unnormalised inverse.  T = double is the reference; T = float is the "plain fp32 radix-2" the forward kernel's error
// is printed next to.
template <class T>
void fft_radix2(Cx<T>* a, int n, int sign) {
  const double pi = 3.14159265358979323846264338327950288;
  std::vector<Cx<T>> w(n / 2);
  for (int k = 0; k < n / 2; k++) w[k] = Cx<T>{(T)std::cos(2.0 * pi * k / n), (T)(sign * std::sin(2.0 * pi * k / n))};
  for (int i = 1, j = 0; i < n; i++) {
    int bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) {
      const Cx<T> t = a[i];
      a[i] = a[j];
      a[j] = t;
    }
  }
  for (int len = 2; len <= n; len <<= 1) {
    const int half = len / 2, step = n / len;
    for (int i = 0; i < n; i += len)
      for (int k = 0; k < half; k++) {
        const Cx<T> tw = w[k * step], u = a[i + k], v = a[i + k + half];
        const Cx<T> t{v.re * tw.re - v.im * tw.im, v.re * tw.im + v.im * tw.re};
        a[i + k] = Cx<T>{u.re + t.re, u.im + t.im};
        a[i + k + half] = Cx<T>{u.re - t.re, u.im - t.im};
      }
  }
}

// bins 0 .. 8192 of the 16,384-point DFT of a real window -> the packed frame: position 0 = (X[0], X[8192]) (both real), position
// 2 j = bin j, position 2 j + 1 = bin 4096 + j
template <class T>
void pack_bins(const Cx<T>* X, Cx<T>* packed) {
  for (int j = 0; j < NB / 2; j++) {
    packed[2 * j] = X[j];
    packed[2 * j + 1] = X[NB / 2 + j];
  }
  packed[0] = Cx<T>{X[0].re, X[NB].re};
}
template <class T>
std::vector<Cx<T>> spectrum_t(const T* window) {
  std::vector<Cx<T>> a(N);
  for (int i = 0; i < N; i++) a[i] = Cx<T>{window[i], (T)0};
  fft_radix2(a.data(), N, -1);
  std::vector<Cx<T>> packed(NB);
  pack_bins(a.data(), packed.data());
  return packed;
}
inline std::vector<cd> ref_spectrum(const double* window) { return spectrum_t<double>(window); }

// ---- forward ----------------------------------------------------------------------------------------------------------------
struct XRow {   // CoarseXRow without the device's bookkeeping
  const float* hist = nullptr;   // the hist_len samples in front of the chunk (nullptr = zeros)
  const float* in = nullptr;     // the chunk (nullptr = zeros)
  int64_t nvalid = 0;            // samples of `in`; zeros beyond
  int n_frames = 0;
  int u0 = 0;                    // window index of frame 0
  int64_t hist_len = 0;
  int flags = 0;                 // bit 0: the second half of every window is zero
  float scale = 1.f;
};
// sample s of history ++ chunk (s < 0: history)
inline double row_sample(const XRow& r, int64_t s) {
  if (s < 0) return r.hist && r.hist_len + s >= 0 ? (double)r.hist[r.hist_len + s] : 0.0;
  return r.in && s < r.nvalid ? (double)r.in[s] : 0.0;
}
// window u covers samples [(u - 1) CB, (u + 1) CB)
inline void row_window(const XRow& r, int u, double* w) {
  for (int i = 0; i < N; i++) {
    const bool second = i >= CB;
    w[i] = (second && (r.flags & 1)) ? 0.0 : row_sample(r, (int64_t)(u - 1) * CB + i) * (double)r.scale;
  }
}
// frame f of the row (window u0 + f): twice the packed spectrum of the scaled window
inline std::vector<cd> ref_fwd_frame(const XRow& r, int f) {
  std::vector<double> w(N);
  row_window(r, r.u0 + f, w.data());
  std::vector<cd> p = ref_spectrum(w.data());
  for (cd& v : p) v = cd{2.0 * v.re, 2.0 * v.im};
  return p;
}
inline std::vector<cd> ref_fwd(const XRow& r) {   // [n_frames][NB]
  std::vector<cd> out((size_t)r.n_frames * NB);
  for (int f = 0; f < r.n_frames; f++) {
    const std::vector<cd> p = ref_fwd_frame(r, f);
    std::memcpy(out.data() + (size_t)f * NB, p.data(), sizeof(cd) * NB);
  }
  return out;
}

// ---- multiply-accumulate ----------------------------------------------------------------------------------------------------
// Y[c][t] = sum over terms sum_{p < P} X_term[t - p] . H_c[p]; position 0 is the element-wise product of two pairs of reals; X[u] = 0
// for u outside [u_lo, u_hi].  T = float: the arrays as the device holds them; T = double: the reference's own.
template <class T>
struct MacTerm {
  const Cx<T>* X;        // the frame buffer
  int64_t frame_u0;      // frame of the signal's window u = 0 (window u: frame_u0 + u; only windows in [u_lo, u_hi] are read)
  const Cx<T>* h[16];    // per column: [P][NB]
};
template <class T>
struct MacJob {
  int P = 0, t0 = 0, n_t = 0, u_lo = 0, u_hi = 0;
  std::vector<MacTerm<T>> terms;
};
// products of one (column, block) of a job: y[NB] (and, if asked for, sum |X| |H| per bin -- |.| the complex modulus; position 0: per
// real -- and the number of products accumulated)
template <class T>
void ref_mac(const MacJob<T>& J, int c, int t, cd* y, double* mag = nullptr, int* nprod = nullptr) {
  for (int b = 0; b < NB; b++) y[b] = cd{0.0, 0.0};
  if (mag)
    for (int b = 0; b < 2 * NB; b++) mag[b] = 0.0;
  int n = 0;
  for (const MacTerm<T>& term : J.terms)
    for (int p = 0; p < J.P; p++) {
      const int u = J.t0 + t - p;
      if (u < J.u_lo || u > J.u_hi) continue;
      n++;
      const Cx<T>* x = term.X + (term.frame_u0 + u) * NB;
      const Cx<T>* h = term.h[c] + (size_t)p * NB;
      for (int b = 1; b < NB; b++) {
        const double xr = x[b].re, xi = x[b].im, hr = h[b].re, hi = h[b].im;
        y[b].re += xr * hr - xi * hi;
        y[b].im += xr * hi + xi * hr;
      }
      y[0].re += (double)x[0].re * (double)h[0].re;
      y[0].im += (double)x[0].im * (double)h[0].im;
      if (mag) {
        for (int b = 1; b < NB; b++) {
          const double xr = x[b].re, xi = x[b].im, hr = h[b].re, hi = h[b].im;
          const double m = std::sqrt((xr * xr + xi * xi) * (hr * hr + hi * hi));
          mag[2 * b] += m;
          mag[2 * b + 1] += m;
        }
        mag[0] += std::fabs((double)x[0].re * (double)h[0].re);
        mag[1] += std::fabs((double)x[0].im * (double)h[0].im);
      }
    }
  if (nprod) *nprod = n;
}

// ---- inverse ----------------------------------------------------------------------------------------------------------------
struct OutDesc {   // CoarseOut without the device's bookkeeping
  int64_t nvalid = 0;
  std::vector<int> rows;           // the Y rows summed
  const float* tail_in = nullptr;
  bool tail_out = false;
  int64_t tail_len = 0;
  int n_y = 0;
};
// samples [CB, 2 CB) of the unnormalised inverse transform of a packed frame
inline void inv_block(const cd* packed, double* out) {
  std::vector<cd> a(N);
  for (int j = 0; j < NB / 2; j++) {
    a[j] = packed[2 * j];
    a[NB / 2 + j] = packed[2 * j + 1];
  }
  a[0] = cd{packed[0].re, 0.0};
  a[NB] = cd{packed[0].im, 0.0};
  for (int k = 1; k < NB; k++) a[N - k] = cd{a[k].re, -a[k].im};
  fft_radix2(a.data(), N, +1);
  for (int i = 0; i < CB; i++) out[i] = a[CB + i].re;
}
// v[i] = y[i] (0 for coarse blocks >= n_y) + tail_in[i] (i < tail_len); out[i] = v[i], i < nvalid; tail_out[i - nvalid] = v[i],
// nvalid <= i < nvalid + tail_len.  Y: [rows][y_frames][NB].  Returns v over [0, nvalid + (tail_out ? tail_len : 0)).
template <class T>
std::vector<double> ref_inv(const OutDesc& o, const Cx<T>* Y, int y_frames) {
  const int64_t send = o.nvalid + (o.tail_out ? o.tail_len : 0);
  std::vector<double> v((size_t)send, 0.0);
  std::vector<cd> sum(NB);
  std::vector<double> blk(CB);
  for (int tb = 0; (int64_t)tb * CB < send; tb++) {
    if (tb < o.n_y) {
      for (cd& s : sum) s = cd{0.0, 0.0};
      for (int row : o.rows) {
        const Cx<T>* y = Y + ((size_t)row * y_frames + tb) * NB;
        for (int b = 0; b < NB; b++) {
          sum[b].re += (double)y[b].re;
          sum[b].im += (double)y[b].im;
        }
      }
      inv_block(sum.data(), blk.data());
      for (int i = 0; i < CB && (int64_t)tb * CB + i < send; i++) v[(size_t)tb * CB + i] = blk[i];
    }
  }
  if (o.tail_in)
    for (int64_t i = 0; i < o.tail_len && i < send; i++) v[(size_t)i] += (double)o.tail_in[i];
  return v;
}

// ---- pre-mix, history -------------------------------------------------------------------------------------------------------
// out[f] = sum over the terms of in_t[f]; sumabs[f] = sum |in_t[f]| (what the bound of the compensated sum is relative to)
inline void ref_premix(const std::vector<const float*>& in, int64_t n, double* out, double* sumabs) {
  for (int64_t f = 0; f < n; f++) {
    double s = 0.0, a = 0.0;
    for (const float* p : in) {
      s += (double)p[f];
      a += std::fabs((double)p[f]);
    }
    out[f] = s;
    sumabs[f] = a;
  }
}
// the last hist_len samples of [old history (hist_len) | this chunk's input (n)]
inline std::vector<float> ref_hist(const float* old_hist, const float* in, int64_t hist_len, int64_t n) {
  std::vector<float> h((size_t)hist_len);
  for (int64_t i = 0; i < hist_len; i++) {
    const int64_t s = i + n;
    h[(size_t)i] = s < hist_len ? (old_hist ? old_hist[s] : 0.f) : (in ? in[s - hist_len] : 0.f);
  }
  return h;
}

}  // namespace coarse_ref
