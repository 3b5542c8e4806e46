"""Float64 model of SpatialPannerNode with occlusion and three-band transmission (option "spatial_occlusion") -- written from the
definition in DESIGN.md section 2e, "Occlusion and transmission", not from the kernel.  Geometry and HRIR selection are those of
tests/_spatial_model.py; the render loop is restated here with the plain gain s, the processed input x' and the run / state rules.

The occlusion arithmetic (band factors, normalisation, triple) is float32, operation for operation, and so are the band filters'
coefficients (rounded once from double); the filters, the ramp of the triple, the mix and everything behind them are float64.
"""
import math

import numpy as np

from tests._spatial_model import B, IDENTITY, INVERSE, f32, geometry, select

EQ_IDENTITY = (f32(1.0), f32(0.0), f32(0.0))
OCCLUSION_DEFAULTS = dict(occlusion=0.0, transmissionLow=0.0, transmissionMid=0.0, transmissionHigh=0.0)   # SpatialPannerNode.cs:94-114


def occlusion(occ, t_low, t_mid, t_high):
    """-> (s, (cM, cL, cH)) in float32: k_i = (1 - occ) + occ t_i for occ > 0 (else 1), s = max k, e = k / s (1 where s == 0)"""
    occ, t = f32(occ), [f32(t_low), f32(t_mid), f32(t_high)]
    k = [f32(1.0)] * 3
    if occ > f32(0.0):
        open_ = f32(f32(1.0) - occ)
        k = [f32(open_ + f32(occ * ti)) for ti in t]
    s = max(k)
    e = [f32(ki / s) for ki in k] if s != f32(0.0) else [f32(1.0)] * 3
    return s, (e[1], f32(e[0] - e[1]), f32(e[2] - e[1]))


def bands(sample_rate):
    """one-pole low-pass at min(800, 0.45 sr) Hz and high-pass at min(8000, 0.45 sr) Hz, bilinear, each coefficient rounded once to
    float32 -> ((b0, b1, a1) low, (b0, b1, a1) high) as Python floats"""
    sr = float(sample_rate)
    kl = math.tan(math.pi * min(800.0, 0.45 * sr) / sr)
    kh = math.tan(math.pi * min(8000.0, 0.45 * sr) / sr)
    r = lambda v: float(f32(v))
    low = (r(kl / (1.0 + kl)), r(kl / (1.0 + kl)), r((kl - 1.0) / (1.0 + kl)))
    high = (r(1.0 / (1.0 + kh)), -r(1.0 / (1.0 + kh)), r((kh - 1.0) / (1.0 + kh)))
    return low, high


def direct(x, triples, silent=None, sample_rate=48000, state=None):
    """x' of x [C][N] (float64): per processed block the triple ramps from the previous processed block's to the block's own
    (w_n = (n + 1) / 128; the first processed block after creation or silence uses its own alone).  A block is active when either
    triple is not the identity; the band filters run in active blocks only, from zero state at the first block of a run; a block that
    is not active is x itself.  `state`: a dict that carries (previous triple, per-channel run-is-open and filter states) from one
    call to the next."""
    x = np.atleast_2d(np.asarray(x, np.float64))
    C, n = x.shape
    nb = n // B
    silent = np.zeros(nb, bool) if silent is None else np.asarray(silent, bool)
    (lb0, lb1, la1), (hb0, hb1, ha1) = bands(sample_rate)
    out = x.copy()
    st = state if state is not None else {}
    prev = st.get("prev")
    open_ = st.get("open", [False] * C)
    z = st.get("z", [[0.0, 0.0] for _ in range(C)])
    w = (np.arange(B) + 1) / float(B)
    for b in range(nb):
        if silent[b]:
            prev = None
            open_ = [False] * C
            continue
        cur = tuple(f32(v) for v in triples[b])
        pr = cur if prev is None else prev
        active = cur != EQ_IDENTITY or pr != EQ_IDENTITY
        if active:
            cm, cl, chh = (float(pr[i]) + w * (float(cur[i]) - float(pr[i])) for i in range(3))
            for c in range(C):
                zl, zh = z[c] if open_[c] else (0.0, 0.0)
                seg = x[c, b * B:(b + 1) * B]
                lo, hi = np.empty(B), np.empty(B)
                for i in range(B):
                    xi = seg[i]
                    lo[i] = yl = lb0 * xi + zl
                    zl = lb1 * xi - la1 * yl
                    hi[i] = yh = hb0 * xi + zh
                    zh = hb1 * xi - ha1 * yh
                z[c] = [zl, zh]
                out[c, b * B:(b + 1) * B] = cm * seg + cl * lo + chh * hi
        open_ = [active] * C
        prev = cur
    st.update(prev=prev, open=open_, z=z)
    return out


def block_occlusion(p):
    q = dict(OCCLUSION_DEFAULTS)
    q.update({k: p[k] for k in OCCLUSION_DEFAULTS if k in p})
    return occlusion(q["occlusion"], q["transmissionLow"], q["transmissionMid"], q["transmissionHigh"])


def render(x, hrir, A, params, model=INVERSE, listener=IDENTITY, silent=None, sample_rate=48000):
    """tests/_spatial_model.render with the stage in front: g_b = f32(g * s), m and the dry path read x'.  params: one dict per block
    (or one for all), which may hold occlusion / transmissionLow / Mid / High beside the geometry's parameters.  -> float64 [2][N]"""
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
    occ = [block_occlusion(p) for p in params]
    xp = direct(x, [o[1] for o in occ], silent, sample_rate)
    m = (0.5 * (xp[0] + xp[1])) if stereo else xp[0].copy()
    dry = xp if stereo else np.stack([xp[0], xp[0]])
    for b in range(nb):
        if silent[b]:
            m[b * B:(b + 1) * B] = 0.0
    mp = np.concatenate([np.zeros(T), m])[-(len(m) + T - 1):] if T > 1 else m
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
        direction, g = geometry({k: v for k, v in p.items() if k not in OCCLUSION_DEFAULTS}, model, listener)
        g = f32(g * occ[b][0])
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
