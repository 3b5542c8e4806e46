"""The float64 model of option "ir_resample" ("Impulse responses at another sample rate"): the band-limited
conversion of an impulse response or an HRIR set from the buffer's rate fi to the context's rate fo.  Written from the definition,
independently of graphaudio_amd/csrc/ga_ir_resample.hpp: np.sinc, np.i0, one matrix of taps per phase.

  g = gcd(fi, fo), L = fo / g, D = fi / g;  rho = R min(1, fo / fi), W = ceil(Z / rho);  M = (N L + D - 1) // D
  h(tau) = rho sinc(rho tau) I0(BETA sqrt(1 - v^2)) / I0(BETA),  v = rho tau / Z,  0 for |v| >= 1
  y[m] = (fi / fo) sum_j x[q - W + 1 + j] h(r / L + W - 1 - j),  q, r = divmod(m D, L),  j = 0 .. 2W-1, terms outside the row skipped
"""
import math
from collections import namedtuple

import numpy as np

Z = 64
BETA = 12.0
R = 0.94
MAX_TABLE = 1 << 22

Plan = namedtuple("Plan", "fi fo L D W rho")


def plan(fi, fo):
    """The plan of a rate pair, or None where the table L x 2W would exceed 2^22 entries."""
    g = math.gcd(fi, fo)
    L, D = fo // g, fi // g
    rho = R * min(1.0, fo / fi)
    W = int(math.ceil(Z / rho))
    if L * 2 * W > MAX_TABLE:
        return None
    return Plan(fi, fo, L, D, W, rho)


def out_length(n, p):
    return (n * p.L + p.D - 1) // p.D


def kernel(p, tau):
    tau = np.asarray(tau, dtype=np.float64)
    v = p.rho * tau / Z
    inside = np.abs(v) < 1.0
    win = np.i0(BETA * np.sqrt(np.where(inside, 1.0 - v * v, 0.0))) / np.i0(BETA)
    return np.where(inside, p.rho * np.sinc(p.rho * tau) * win, 0.0)


def resample(x, fi, fo):
    """x: (..., N) array at rate fi -> float64 array (..., M) at rate fo."""
    p = plan(fi, fo)
    assert p is not None, (fi, fo)
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    m = np.arange(out_length(n, p), dtype=np.int64)
    q, r = np.divmod(m * p.D, p.L)
    j = np.arange(2 * p.W, dtype=np.int64)
    k = q[:, None] - p.W + 1 + j[None, :]                      # (M, 2W) input frames
    taps = kernel(p, r[:, None] / p.L + (p.W - 1 - j)[None, :])
    ok = (k >= 0) & (k < n)
    taps = np.where(ok, taps, 0.0)
    xs = x[..., np.clip(k, 0, max(n - 1, 0))]                  # (..., M, 2W)
    return (fi / fo) * np.sum(xs * taps, axis=-1)
