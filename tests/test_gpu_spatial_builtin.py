"""The built-in HRIR set of SpatialPannerNode on the device (options "spatial_builtin_hrir" / "spatial_head_radius"; DESIGN.md section
2e, "The built-in set"): spatial_head_kernel's taps against the float64 model of tests/_spatial_head_model.py, and nodes that render
on the set against tests/_spatial_model.py fed the model's set with A = 72.

Bounds.  Taps read through a render: |device - model| <= max(one float32 ulp at the model's value, 2^-40), the host test's derived
bound (tests/_spatial_head_model.bound) -- a unit impulse from a grid direction at g = 1 puts the ears' taps into the output rows
without an operation that rounds.  Renders: the node's existing bound, max-abs <= 1e-5 x max(1, peak of the model's output)
(tests/test_gpu_spatial.check).  Pieces across render calls are bit for bit.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from graphaudio_amd import (ArgumentOutOfRangeException, AudioBufferSourceNode, HrirSet, NotSupportedException, OfflineAudioContext,
                            PlayableAudioBuffer, SpatialPannerNode)
from tests import _graphs as G
from tests import _spatial_direct_model as DM
from tests import _spatial_head_model as H
from tests import _spatial_model as M
from tests.test_gpu_spatial import M_rms, check, noise_set, render, set_params
from tests.test_gpu_spatial_signals import const, guard, modulated

SR = 48000
B = 128
f32 = np.float32
NB = 24


def new_context(sr=SR, radius=None, builtin=1, **opts):
    ctx = OfflineAudioContext(sr)
    if builtin is not None:
        ctx.SetOption("spatial_builtin_hrir", builtin)
    if radius is not None:
        ctx.SetOption("spatial_head_radius", radius)
    for k, v in opts.items():
        ctx.SetOption(k, v)
    return ctx


def source(ctx, x, sr=SR, when=0.0, stop=None):
    """tests/test_gpu_spatial.source at the context's rate: x followed by 256 zeros that are never reached"""
    s = AudioBufferSourceNode(ctx)
    x = np.asarray(x, np.float32)
    x = np.concatenate([x, np.zeros(x.shape[:-1] + (256,), np.float32)], axis=-1)
    s.Buffer = PlayableAudioBuffer.FromMonoArray(x, sr) if x.ndim == 1 else PlayableAudioBuffer.FromStereoArrays(x[0], x[1], sr)
    s.Start(when)
    if stop is not None:
        s.Stop(stop)
    return s


def orbit(nb):
    """one position per block: the azimuth crosses the 360 / 0 seam, the elevation angle runs over +90 (block 2) and on through 270 = -90
    (block 20): both poles"""
    pts = []
    for b in range(nb):
        az, el = math.radians(335.0 + 4.0 * b), math.radians(70.0 + 10.0 * b)
        r = 1.5 + 0.05 * b
        d = (math.sin(az) * math.cos(el), math.sin(el), -math.cos(az) * math.cos(el))
        pts.append(tuple(float(f32(r * c)) for c in d))
    return pts


def put_on_orbit(p, pts, bt, first=0):
    for b, (px, py, pz) in enumerate(pts):
        if b >= first:
            p.PositionX.SetValueAtTime(px, bt[b])
            p.PositionY.SetValueAtTime(py, bt[b])
            p.PositionZ.SetValueAtTime(pz, bt[b])
    return [dict(positionX=px, positionY=py, positionZ=pz) for px, py, pz in pts]


def test_orbit_crosses_the_seam_and_both_poles():
    els, azs = [], []
    for px, py, pz in orbit(NB):
        az, el = M.azimuth_elevation(M.geometry(dict(positionX=px, positionY=py, positionZ=pz))[0])
        els.append(el)
        azs.append(az)
    rings = [int(math.floor((el + 90.0) / 180.0 * (H.E - 1))) for el in els]
    assert max(rings) >= H.E - 2 and min(rings) == 0                 # the cells next to both poles
    assert any(a > 300.0 for a in azs) and any(a < 60.0 for a in azs)


# ---- 1. the options; refused without, rendered with ------------------------------------------------------------------------------

def test_options_and_refusal_then_render():
    frames = 12 * B
    x = G.voice(51, frames)
    values = dict(positionX=1.0, positionY=-0.5, positionZ=0.8)
    ctx = OfflineAudioContext(SR)
    ctx.SetOption("spatial_builtin_hrir", 1)
    ctx.SetOption("spatial_builtin_hrir", 0)
    for key, bad in (("spatial_builtin_hrir", 2), ("spatial_builtin_hrir", -1), ("spatial_head_radius", 0.03), ("spatial_head_radius", 0.3)):
        with pytest.raises(ArgumentOutOfRangeException):
            ctx.SetOption(key, bad)
    for ok in (0.04, 0.2, H.DEFAULT_RADIUS):
        ctx.SetOption("spatial_head_radius", ok)
    s = source(ctx, x)
    p = SpatialPannerNode(ctx)
    p.HrirAzimuths = 4            # (the node's own count is not the built-in set's)
    set_params(p, values)
    s.Connect(p).Connect(ctx.Destination)
    out = np.zeros((2, frames), np.float32)
    with pytest.raises(NotSupportedException, match="no HRIR set assigned"):
        ctx.Render(out, frames, 0)
    assert ctx.CurrentBlock == 0
    ctx.SetOption("spatial_builtin_hrir", 1)
    ctx.Render(out, frames, 0)
    ctx.Dispose()
    check(out, M.render(x, H.hrir(SR), H.A, values), "refused, then on the built-in set")


# ---- 2. the taps, read through a render ------------------------------------------------------------------------------------------

AXIS_POSITIONS = [(0, 0, -1), (1, 0, 0), (0, 0, 1), (-1, 0, 0), (0, 1, 0), (0, -1, 0)]


@pytest.mark.parametrize("sr,radius", [(48000, 0.0875), (8000, 0.0875), (96000, 0.0875), (48000, 0.05), (48000, 0.15)])
def test_taps_through_a_render(sr, radius):
    model = H.hrir(sr, radius)
    T = model.shape[2]
    assert T == H.taps(sr, radius)
    frames = (-(-T // B) + 1) * B
    x = np.zeros(frames, np.float32)
    x[0] = 1.0
    worst = 0.0
    seen = set()
    for pos in AXIS_POSITIONS:
        values = dict(positionX=float(pos[0]), positionY=float(pos[1]), positionZ=float(pos[2]))
        direction, g = M.geometry(values)
        idx, w = M.select(direction, H.A, H.E)
        assert g == f32(1.0) and tuple(float(v) for v in w) == (1.0, 0.0, 0.0, 0.0), (pos, g, w)   # tap for tap: no gain, one direction
        seen.add(idx[0])
        ctx = new_context(sr, radius)
        s = source(ctx, x, sr)
        p = SpatialPannerNode(ctx)
        set_params(p, values)
        s.Connect(p).Connect(ctx.Destination)
        out = render(ctx, frames)
        ctx.Dispose()
        assert not out[:, T:].any(), pos
        for ear in range(2):
            want = model[idx[0], ear]
            err = np.abs(out[ear, :T].astype(np.float64) - want.astype(np.float64))
            ratio = float(np.max(err / H.bound(want)))
            worst = max(worst, ratio)
            print(f"sr {sr} a {radius} source at {pos} -> direction {idx[0]} ear {ear}: max |device - model| {err.max():.3e}, {ratio:.3f} x bound")
            assert np.all(err <= H.bound(want)), (pos, ear, int(np.argmax(err - H.bound(want))))
        assert M_rms(out[:, :T]) > 1e-3
    assert len(seen) >= 5       # (the poles may share an azimuth index; the four horizontal axes and the two rings are distinct)
    print(f"sr {sr} a {radius}: T {T}, worst {worst:.3f} x bound")


# ---- 3. off-grid and moving sources ----------------------------------------------------------------------------------------------

def static_directions():
    rng = np.random.default_rng(31415)
    out = []
    for _ in range(4):
        v = rng.standard_normal(3)
        v = v / np.linalg.norm(v) * rng.uniform(1.2, 3.0)
        out.append(tuple(float(f32(c)) for c in v))
    return out


def inputs(stereo, frames, seed):
    return np.stack([G.voice(seed, frames), G.voice(seed + 1, frames)]) if stereo else G.voice(seed, frames)


@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
def test_static_off_grid_sources(stereo):
    frames = NB * B
    h = H.hrir(SR)
    x = inputs(stereo, frames, 61)
    for i, pos in enumerate(static_directions()):
        values = dict(positionX=pos[0], positionY=pos[1], positionZ=pos[2], spatialBlend=0.6 if stereo else 1.0)
        _, w = M.select(M.geometry(values)[0], H.A, H.E)
        assert sum(1 for v in w if v > 0) == 4          # off the grid: four directions take part
        ctx = new_context()
        s = source(ctx, x)
        p = SpatialPannerNode(ctx)
        set_params(p, values)
        s.Connect(p).Connect(ctx.Destination)
        out = render(ctx, frames)
        ctx.Dispose()
        check(out, M.render(x, h, H.A, values), f"static direction {i}, stereo={stereo}")


def orbit_scene(ctx, x):
    bt = M.block_times(NB, SR)
    s = source(ctx, x)
    p = SpatialPannerNode(ctx)
    if np.ndim(x) == 2:
        p.SpatialBlend.Value = 0.6
    params = put_on_orbit(p, orbit(NB), bt)
    if np.ndim(x) == 2:
        params = [dict(q, spatialBlend=0.6) for q in params]
    s.Connect(p).Connect(ctx.Destination)
    return (s, p), params


@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
def test_orbit_against_the_model_and_in_pieces(stereo):
    frames = NB * B
    x = inputs(stereo, frames, 63)
    outs = []
    for pieces in (None, [3 * B, 1 * B, 7 * B + 40, 5 * B - 40, 2 * B]):      # uneven pieces, two of them inside a block
        ctx = new_context()
        hold, params = orbit_scene(ctx, x)
        outs.append(render(ctx, frames, pieces))
        ctx.Dispose()
    check(outs[0], M.render(x, H.hrir(SR), H.A, params), f"orbit, stereo={stereo}")
    assert np.array_equal(outs[0], outs[1])


# ---- 4. explicit versus built-in ---------------------------------------------------------------------------------------------------

def test_explicit_set_agrees_with_the_built_in_one():
    frames = NB * B
    x = inputs(False, frames, 65)
    outs = []
    for explicit in (False, True):
        ctx = new_context(builtin=0 if explicit else 1)
        hold, params = orbit_scene(ctx, x)
        if explicit:
            hs = HrirSet.SphericalHead(SR)
            hold[1].HrirAzimuths = hs.Azimuths
            hold[1].Hrir = hs
        outs.append(render(ctx, frames))
        ctx.Dispose()
    ref = M.render(x, H.hrir(SR), H.A, params)
    check(outs[0], ref, "built-in")
    check(outs[1], ref, "explicit SphericalHead")
    scale = max(1.0, float(np.max(np.abs(ref))))
    diff = float(np.max(np.abs(outs[0].astype(np.float64) - outs[1])))
    print(f"explicit against built-in: max-abs difference {diff:.3e}")
    assert diff <= 1e-5 * scale


def test_both_kinds_in_one_level():
    """a node with a set of its own and a node on the built-in set side by side; the first source stops after block 13, the second starts
    at block 6: blocks 0 .. 5 are the first node alone, 14 .. 23 the second alone, 6 .. 13 their sum"""
    frames = NB * B
    bt = M.block_times(NB, SR)
    own = noise_set(6 * 3, 64, 5)
    xa, xb = G.voice(71, frames), G.voice(72, frames - 6 * B)
    va = dict(positionX=1.3, positionY=0.7, positionZ=-2.1)
    vb = dict(positionX=-0.8, positionY=0.3, positionZ=-1.1)
    ctx = new_context()
    sa = source(ctx, xa, when=0.0, stop=bt[14])
    sb = source(ctx, xb, when=bt[6])
    pa = SpatialPannerNode(ctx)
    pa.HrirAzimuths = 6
    pa.Hrir = HrirSet.FromArray(own, SR)
    pb = SpatialPannerNode(ctx)
    set_params(pa, va)
    set_params(pb, vb)
    sa.Connect(pa).Connect(ctx.Destination)
    sb.Connect(pb).Connect(ctx.Destination)
    out = render(ctx, frames)
    ctx.Dispose()
    ina = np.zeros(frames, np.float32)
    ina[:14 * B] = xa[:14 * B]
    inb = np.zeros(frames, np.float32)
    inb[6 * B:] = xb
    sil_a = np.arange(NB) >= 14
    sil_b = np.arange(NB) < 6
    ref_a = M.render(ina, own, 6, va, silent=sil_a)
    ref_b = M.render(inb, H.hrir(SR), H.A, vb, silent=sil_b)
    check(out[:, :6 * B], ref_a[:, :6 * B], "own set alone")
    check(out[:, 14 * B:], ref_b[:, 14 * B:], "built-in set alone")
    check(out, ref_a + ref_b, "both kinds")


# ---- 5. transitions between render calls -------------------------------------------------------------------------------------------

def continuation(x, params, start, stop, h, A):
    """blocks [start, stop) as a render that continues behind a changed set: the input history stays, the first block does not fade"""
    return M.render(x[start * B:stop * B], h, A, params[start:stop], history=M.mono_mix(x[:start * B]) if start else None)


def test_own_set_assigned_and_cleared_between_render_calls():
    frames = NB * B
    x = G.voice(81, frames)
    small = noise_set(4, 129, 82)
    ctx = new_context()
    (s, p), params = orbit_scene(ctx, x)
    out = np.zeros((2, frames), np.float32)
    ctx.Render(out, 7 * B, 0)
    p.HrirAzimuths = 4
    p.Hrir = HrirSet.FromArray(small, SR)
    ctx.Render(out, 8 * B, 7 * B)
    p.Hrir = None                                  # ga_convolver_set_buffer(node, -1): back on the built-in set, 72 azimuths again
    ctx.Render(out, 9 * B, 15 * B)
    ctx.Dispose()
    built = H.hrir(SR)
    ref = np.concatenate([continuation(x, params, 0, 7, built, H.A), continuation(x, params, 7, 15, small, 4),
                          continuation(x, params, 15, NB, built, H.A)], axis=1)
    # (a fade into the first block of a piece would be heard: the model with the fade differs)
    faded = M.render(x, built, H.A, params)
    assert np.max(np.abs(faded[:, 15 * B:16 * B] - ref[:, 15 * B:16 * B])) > 1e-4     # (the check's bound is 1e-5)
    check(out, ref, "built-in -> own -> built-in")


def test_radius_changed_between_render_calls():
    frames = NB * B
    x = G.voice(83, frames)
    ctx = new_context()
    (s, p), params = orbit_scene(ctx, x)
    out = np.zeros((2, frames), np.float32)
    ctx.Render(out, 9 * B, 0)
    ctx.SetOption("spatial_head_radius", 0.06)
    ctx.Render(out, 15 * B, 9 * B)
    ctx.Dispose()
    a, b = H.hrir(SR), H.hrir(SR, 0.06)
    assert a.shape[2] != b.shape[2]
    ref = np.concatenate([continuation(x, params, 0, 9, a, H.A), continuation(x, params, 9, NB, b, H.A)], axis=1)
    assert np.max(np.abs(ref[:, 9 * B:] - M.render(x, a, H.A, params)[:, 9 * B:])) > 1e-3     # the other head is heard
    check(out, ref, "radius 0.0875 -> 0.06")


def test_option_off_and_on_between_render_calls():
    frames = NB * B
    x = G.voice(85, frames)
    ctx = new_context()
    (s, p), params = orbit_scene(ctx, x)
    out = np.zeros((2, frames), np.float32)
    ctx.Render(out, 9 * B, 0)
    ctx.SetOption("spatial_builtin_hrir", 0)
    with pytest.raises(NotSupportedException, match="no HRIR set assigned"):
        ctx.Render(out, 15 * B, 9 * B)
    assert ctx.CurrentBlock == 9
    ctx.SetOption("spatial_builtin_hrir", 1)
    ctx.Render(out, 15 * B, 9 * B)
    ctx.Dispose()
    h = H.hrir(SR)
    ref = np.concatenate([continuation(x, params, 0, 9, h, H.A), continuation(x, params, 9, NB, h, H.A)], axis=1)
    check(out, ref, "option off, refused, on again")


# ---- 6. memory ---------------------------------------------------------------------------------------------------------------------

def test_radius_changes_do_not_accumulate_device_memory():
    """twenty remakes of the set (two radii in turn, sets of the same stored size), a block rendered after each: the copy a remake
    replaces is freed once the stream is idle"""
    x = G.voice(87, 24 * B)
    ctx = new_context()
    s = source(ctx, x)
    p = SpatialPannerNode(ctx)
    set_params(p, dict(positionX=1.0, positionY=-0.5, positionZ=0.8))
    s.Connect(p).Connect(ctx.Destination)
    out = np.zeros((2, 24 * B), np.float32)
    ctx.Render(out, B, 0)
    used = []
    for i in range(20):
        ctx.SetOption("spatial_head_radius", 0.08 if i % 2 == 0 else 0.0875)
        ctx.Render(out, B, (i + 1) * B)
        used.append(ctx.GetStats()["device_bytes_in_use"])
    ctx.Dispose()
    print("device bytes after each radius change:", used)
    assert M_rms(out[:, :21 * B]) > 1e-3
    assert max(used[2:]) <= used[1], used


# ---- 7. with the other spatial options ----------------------------------------------------------------------------------------------

def test_signal_driven_node_on_the_built_in_set():
    frames = 12 * B
    x = G.voice(51, frames)
    values = dict(positionX=1.0, positionY=-0.5, positionZ=0.8)
    ctx = new_context(spatial_param_signals=1)
    s = source(ctx, x)
    p = SpatialPannerNode(ctx)
    set_params(p, values)
    s.Connect(p).Connect(ctx.Destination)
    c = const(ctx, 0.5)
    c.Connect(p.PositionX)
    out = render(ctx, frames)
    ctx.Dispose()
    want = dict(values, positionX=modulated("positionX", 1.0, 0.5))
    guard(want, 12)
    h = H.hrir(SR)
    ref = M.render(x, h, H.A, want)
    assert np.max(np.abs(ref - M.render(x, h, H.A, values))) > 1e-2      # the signal is heard
    check(out, ref, "signal on positionX, built-in set")


def test_occluded_node_on_the_built_in_set():
    nb = 16
    frames = nb * B
    x = G.voice(61, frames)
    values = dict(positionX=1.0, positionY=-0.5, positionZ=0.8, occlusion=1.0, transmissionLow=0.9, transmissionMid=0.5, transmissionHigh=0.1)
    ctx = new_context(spatial_occlusion=1)
    s = source(ctx, x)
    p = SpatialPannerNode(ctx)
    set_params(p, values)
    s.Connect(p).Connect(ctx.Destination)
    out = render(ctx, frames)
    ctx.Dispose()
    guard({k: v for k, v in values.items() if k in M.PARAM_DEFAULTS}, nb)
    h = H.hrir(SR)
    ref = DM.render(x, h, H.A, values)
    plain = M.render(x, h, H.A, {k: v for k, v in values.items() if k in M.PARAM_DEFAULTS})
    assert np.max(np.abs(ref - float(DM.block_occlusion(values)[0]) * plain)) > 1e-2      # more than a gain: the EQ is heard
    check(out, ref, "wall, built-in set")
