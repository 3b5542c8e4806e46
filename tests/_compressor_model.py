"""DynamicsCompressorNode: the definition of include/graphaudio_hip.h / DESIGN.md section 2g in numpy float64, frame by frame.
The node is this library's own (the reference has none), so this model is what the device is held to: |y - m| <= 2^-22 |m| for every
sample (tests/test_gpu_compressor_kernel.py says where the two ulps come from).  The state yL carries across calls."""
import numpy as np

F32 = np.float32
BLOCK = 128
# (name, default, min, max) in the native parameter order
PARAMS = (("threshold", -24.0, -100.0, 0.0), ("knee", 30.0, 0.0, 40.0), ("ratio", 12.0, 1.0, 20.0),
          ("attack", 0.003, 0.0, 1.0), ("release", 0.25, 0.0, 1.0), ("makeupGain", 0.0, -40.0, 40.0))
TOL = 2.0 ** -22


def block_params(fs, **values):
    """{T, W, R, M, aA, aR} of one block from the parameters' float values: clamped to the range as floats, widened to double."""
    v = {}
    for name, default, mn, mx in PARAMS:
        x = F32(values.pop(name, default))
        v[name] = float(min(max(x, F32(mn)), F32(mx)))
    assert not values, values
    at, rl = v["attack"], v["release"]
    aA = float(np.exp(-1.0 / (at * fs))) if at > 0 else 0.0
    aR = float(np.exp(-1.0 / (rl * fs))) if rl > 0 else 0.0
    return (v["threshold"], v["knee"], v["ratio"], v["makeupGain"], aA, aR)


def level_reduction(a, T, W, R):
    """xL of steps 1 - 4 for an array of linked magnitudes a (float32)."""
    a = np.asarray(a, dtype=F32).astype(np.float64)
    xG = 20.0 * np.log10(np.maximum(a, 1e-6))
    d = xG - T
    with np.errstate(divide="ignore", invalid="ignore"):
        q = d + W / 2.0
        knee = xG + ((1.0 / R - 1.0) * (q * q)) / (2.0 * W)
    yG = np.where(2.0 * d < -W, xG, np.where((W > 0) & (np.abs(2.0 * d) <= W), knee, T + d / R))
    return xG - yG


class Compressor:
    def __init__(self, fs):
        self.fs = fs
        self.yL = 0.0

    def process(self, x, pars):
        """x: [channels][frames] float32 (1 or 2 channels; frames a multiple of 128 when `pars` is a list with one entry per block),
        pars: one block_params tuple or a list of them.  Returns y like x and moves yL."""
        x = np.atleast_2d(np.asarray(x, dtype=F32))
        n = x.shape[1]
        y = np.empty_like(x)
        per_block = isinstance(pars, list)
        for f0 in range(0, n, BLOCK):
            T, W, R, M, aA, aR = pars[f0 // BLOCK] if per_block else pars
            xs = x[:, f0:f0 + BLOCK]
            xL = level_reduction(np.max(np.abs(xs), axis=0), T, W, R)
            yv = np.empty(xs.shape[1])
            yL = self.yL
            for i, v in enumerate(xL.tolist()):
                yL = aA * yL + (1.0 - aA) * v if v > yL else aR * yL + (1.0 - aR) * v
                yv[i] = yL
            self.yL = yL
            g = np.power(10.0, (M - yv) / 20.0).astype(F32)   # the one rounding to float
            y[:, f0:f0 + BLOCK] = xs * g                       # a float product
        return y

    def silence(self, frames, pars):
        """Silent input: xL = 0, the state still moves."""
        per_block = isinstance(pars, list)
        for f in range(frames):
            T, W, R, M, aA, aR = pars[f // BLOCK] if per_block else pars
            yL = self.yL
            self.yL = aA * yL + (1.0 - aA) * 0.0 if 0.0 > yL else aR * yL + (1.0 - aR) * 0.0


def within(y, m):
    """every sample within two float ulps of the model; where the model is exactly 0 the sample is exactly 0"""
    y = np.asarray(y, dtype=np.float64)
    m = np.asarray(m, dtype=np.float64)
    return bool(np.all(np.abs(y - m) <= TOL * np.abs(m)))


def worst(y, m):
    """largest |y - m| / |m| over the samples where the model is not 0 (a figure to print; `within` is the condition)"""
    y = np.asarray(y, dtype=np.float64)
    m = np.asarray(m, dtype=np.float64)
    nz = m != 0
    return float(np.max(np.abs(y[nz] - m[nz]) / np.abs(m[nz]))) if nz.any() else 0.0


def bursts(seed, frames, channels=1, levels_db=(-40.0, -12.0, 0.0), burst=96, gap=40):
    """seeded noise bursts at the given peak levels (dBFS) with silent gaps, float32 [channels][frames]"""
    rng = np.random.default_rng(seed)
    x = np.zeros((channels, frames), dtype=F32)
    f, k = int(rng.integers(0, gap)), 0
    while f < frames:
        n = min(burst + int(rng.integers(0, burst)), frames - f)
        amp = 10.0 ** (levels_db[k % len(levels_db)] / 20.0)
        x[:, f:f + n] = (rng.uniform(-1.0, 1.0, size=(channels, n)) * amp).astype(F32)
        f += n + gap + int(rng.integers(0, gap))
        k += 1
    return x
