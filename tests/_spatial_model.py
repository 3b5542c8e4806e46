"""Float64 model of SpatialPannerNode on a supplied HRIR set -- written from the node's definition (DESIGN.md "SpatialPannerNode")
and from the geometry of GraphAudio.SteamAudio/Nodes/SpatialPannerNode.cs:133-204,263-284, not from the kernel.

Geometry (direction, directivity, distance attenuation) is float32, operation for operation, as in the C#; azimuth, elevation
and the four bilinear weights are computed in double and the weights rounded to float32; filtering and the crossfade are float64.
"""
import math

import numpy as np

f32 = np.float32
B = 128
IDENTITY = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, -1.0))   # origin, right, up, ahead (SteamAudioContext.cs:45-54)
PARAM_DEFAULTS = dict(positionX=0.0, positionY=0.0, positionZ=0.0, orientationX=1.0, orientationY=0.0, orientationZ=0.0,
                      refDistance=1.0, maxDistance=10000.0, rolloffFactor=1.0, coneInnerAngle=360.0, coneOuterAngle=360.0,
                      coneOuterGain=0.0, spatialBlend=1.0)
LINEAR, INVERSE, EXPONENTIAL = 0, 1, 2


def block_times(nblocks, sample_rate=48000, t0=0.0):
    """the accumulated block clock (AudioContextBase.cs:78-79): t += 128 / sampleRate in double"""
    t = [float(t0)]
    for _ in range(nblocks):
        t.append(t[-1] + B / float(sample_rate))
    return t


def linear_ramp(v0, t0, v1, t1, t):
    """AudioParam.InterpolateLinear (AudioParam.cs:220-225)"""
    u = min(max((t - t0) / (t1 - t0), 0.0), 1.0)
    return f32(float(f32(v0)) + float(f32(f32(v1) - f32(v0))) * u)


def listener_from(position, forward, up):
    """SteamAudioContext.SetListener (SteamAudioContext.cs:145-164) in float32: normalise, right = forward x up, ahead = -forward"""
    def norm(v):
        x, y, z = (f32(c) for c in v)
        ln = np.sqrt(f32(f32(x * x + y * y) + z * z))
        return (f32(x / ln), f32(y / ln), f32(z / ln))
    fw, u = norm(forward), norm(up)
    right = (f32(f32(fw[1] * u[2]) - f32(fw[2] * u[1])), f32(f32(fw[2] * u[0]) - f32(fw[0] * u[2])), f32(f32(fw[0] * u[1]) - f32(fw[1] * u[0])))
    return (tuple(f32(c) for c in position), right, u, (f32(-fw[0]), f32(-fw[1]), f32(-fw[2])))


def _clamp(v, lo, hi):   # Math.Clamp's comparison order
    return lo if v < lo else (hi if v > hi else v)


def _dot3(a, b):   # a.X * b.X + a.Y * b.Y + a.Z * b.Z in float32, left to right
    return f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))


def geometry(p, model=INVERSE, listener=IDENTITY):
    """-> (direction in listener space (3 float32), g float32).  `p`: parameter name -> value (missing ones take the defaults)."""
    q = {k: f32(v) for k, v in PARAM_DEFAULTS.items()}
    q.update({k: f32(v) for k, v in p.items()})
    origin, right, up, ahead = [tuple(f32(c) for c in v) for v in listener]
    with np.errstate(all="ignore"):
        w = [f32(q["positionX"] - origin[0]), f32(q["positionY"] - origin[1]), f32(q["positionZ"] - origin[2])]
        distance = f32(np.sqrt(_dot3(w, w)))
        if distance > f32(0.0001):
            inv = f32(f32(1.0) / distance)
            w = [f32(c * inv) for c in w]
            direction = (_dot3(w, right), _dot3(w, up), _dot3(w, ahead))
        else:
            direction = (f32(0), f32(0), f32(-1))
            distance = f32(0)
        directivity = f32(1.0)
        inner, outer, outer_gain = q["coneInnerAngle"], q["coneOuterAngle"], q["coneOuterGain"]
        if inner < f32(360) or outer < f32(360):
            ori = (q["orientationX"], q["orientationY"], q["orientationZ"])
            mag = f32(np.sqrt(_dot3(ori, ori)))
            if mag > f32(0.0001):
                inv = f32(f32(1.0) / mag)
                n = [f32(c * inv) for c in ori]
                dot = _clamp(_dot3(n, [f32(-c) for c in w]), f32(-1), f32(1))
                angle = f32(f32(f32(np.arccos(dot)) * f32(180.0)) / f32(math.pi))
                a = abs(angle)
                hi_, ho = f32(inner * f32(0.5)), f32(outer * f32(0.5))
                if a <= hi_:
                    directivity = f32(1.0)
                elif a >= ho:
                    directivity = outer_gain
                else:
                    t = f32(f32(a - hi_) / f32(ho - hi_))
                    directivity = f32(f32(1.0) + f32(t * f32(outer_gain - f32(1.0))))
        ref, mx, roll = q["refDistance"], q["maxDistance"], q["rolloffFactor"]
        steam = f32(f32(1.0) / max(distance, ref))           # Steam Audio's documented inverse curve: 1 / max(distance, minDistance)
        dc = _clamp(distance, ref, mx)
        if model == LINEAR:
            att = f32(f32(1.0) - f32(f32(roll * f32(dc - ref)) / f32(mx - ref)))
        elif model == INVERSE:
            att = steam
        else:
            att = f32(np.power(f32(dc / ref), f32(-roll)))
        att = _clamp(att, f32(0), f32(1))
        g = f32(att * (directivity if directivity < f32(0.999) else f32(1.0)))
    return direction, g


def azimuth_elevation(direction):
    """degrees, in double from the float32 direction: azimuth 0 = front (-z), +90 = right (+x), in [0, 360)"""
    x, y, z = (float(c) for c in direction)
    az = math.degrees(math.atan2(x, -z))
    if az < 0.0:
        az += 360.0
    el = math.degrees(math.asin(min(max(y, -1.0), 1.0)))
    return az, el


def select(direction, A, E):
    """-> (four direction indices (j0,i0), (j0,i1), (j1,i0), (j1,i1) with d = j * A + i, four float32 weights)"""
    az, el = azimuth_elevation(direction)
    pa = az * A / 360.0
    i0 = int(math.floor(pa))
    fa = pa - i0
    i0 %= A
    i1 = (i0 + 1) % A
    j0 = j1 = 0
    fe = 0.0
    if E > 1:
        pe = (el + 90.0) / 180.0 * (E - 1)
        j0 = min(max(int(math.floor(pe)), 0), E - 1)
        j1 = min(j0 + 1, E - 1)
        fe = 0.0 if j1 == j0 else pe - j0
    idx = (j0 * A + i0, j0 * A + i1, j1 * A + i0, j1 * A + i1)
    w = (f32((1.0 - fe) * (1.0 - fa)), f32((1.0 - fe) * fa), f32(fe * (1.0 - fa)), f32(fe * fa))
    return idx, w


def mono_mix(x, silent=None):
    """the signal the spatial path filters: x (mono) or 0.5 (L + R) (stereo), zeros in silent input blocks"""
    x = np.asarray(x, dtype=np.float64)
    m = (0.5 * (x[0] + x[1])) if x.ndim == 2 else x.copy()
    for b in np.nonzero(np.asarray(silent, bool))[0] if silent is not None else []:
        m[b * B:(b + 1) * B] = 0.0
    return m


def render(x, hrir, A, params, model=INVERSE, listener=IDENTITY, silent=None, history=None):
    """x: [N] (mono) or [2][N] (stereo) input, N a multiple of 128; hrir[d][ear][k] float32; params: one dict per block (or one dict
    for all blocks); silent: per-block flags of a silent INPUT block; history: the mono mix of the frames in front of x (a render
    that continues after the HRIR set was replaced: the input history stays, the first block uses its own filters alone).
    -> float64 [2][N]."""
    x = np.asarray(x, dtype=np.float64)
    stereo = x.ndim == 2
    n = x.shape[-1]
    nb = n // B
    assert nb * B == n
    hrir = np.asarray(hrir, dtype=np.float32)
    D, _, T = hrir.shape
    E = D // A
    assert E * A == D
    if isinstance(params, dict):
        params = [params] * nb
    silent = np.zeros(nb, bool) if silent is None else np.asarray(silent, bool)
    m = (0.5 * (x[0] + x[1])) if stereo else x.copy()
    dry = x if stereo else np.stack([x, x])
    for b in range(nb):
        if silent[b]:
            m[b * B:(b + 1) * B] = 0.0   # the history receives the block's zeros
    hist = np.zeros(0) if history is None else np.asarray(history, np.float64)
    mp = np.concatenate([np.zeros(T), hist, m])[-(len(m) + T - 1):] if T > 1 else m
    out = np.zeros((2, n), np.float64)
    h64 = hrir.astype(np.float64)
    wn = (np.arange(B) + 1) / float(B)
    prev = None

    def apply(desc, b):
        idx, w, g, beta = desc
        seg = mp[b * B:(b + 1) * B + T - 1]
        y = np.zeros((2, B))
        for ear in range(2):
            H = sum(float(w[q]) * h64[idx[q], ear] for q in range(4))
            F = float(g) * float(beta) * H
            y[ear] = np.convolve(seg, F, mode="valid") + float(g) * (1.0 - float(beta)) * dry[ear, b * B:(b + 1) * B]
        return y

    for b in range(nb):
        if silent[b]:
            prev = None
            continue
        p = params[b]
        direction, g = geometry(p, model, listener)
        idx, w = select(direction, A, E)
        beta = f32(p.get("spatialBlend", 1.0))
        desc = (idx, w, g, beta)
        y = apply(desc, b)
        changed = prev is not None and (prev[0] != idx or any(a != c for a, c in zip(prev[1], w)) or prev[2] != g or prev[3] != beta)
        if changed:
            y = (1.0 - wn) * apply(prev, b) + wn * y
        out[:, b * B:(b + 1) * B] = y
        prev = desc
    return out
