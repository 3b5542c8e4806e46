"""SpatialPannerNode on the device (DESIGN.md "SpatialPannerNode") against the float64 model of tests/_spatial_model.py.

Bounds: the delta-set cases are bit for bit; everything else is the project's convolver contract, max-abs <= 1e-5 x max(1, peak of
the model's output).  Measured on an MI355X (printed by every case): at most 6.6e-7 x that scale (T = 512, spatialBlend 1); the delta
cases read the device's gain within 1e-6 relative of the float32 restatement and are then bit for bit.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from graphaudio_amd import (AudioBufferSourceNode, ConstantSourceNode, DistanceModelType, HrirSet, InvalidOperationException,
                            NotSupportedException, OfflineAudioContext, PlayableAudioBuffer, SpatialPannerNode)
from tests import _graphs as G
from tests import _spatial_model as M

SR = 48000
B = 128
f32 = np.float32


def noise_set(D, T, seed):
    """seeded decaying noise, hrir[d][ear][k]"""
    k = np.arange(T)
    return (np.random.default_rng(seed).standard_normal((D, 2, T)) * np.exp(-6.9 * k / T) * 0.5).astype(np.float32)


def source(ctx, x, when=0.0, stop=None):
    """x, followed by 256 zeros that are never reached: the reference clears the block in which a source arrives at the end of its buffer
    (AudioBufferSourceNode.cs:360), so a buffer that ends with the render would lose its last block"""
    s = AudioBufferSourceNode(ctx)
    x = np.asarray(x, np.float32)
    x = np.concatenate([x, np.zeros(x.shape[:-1] + (256,), np.float32)], axis=-1)
    s.Buffer = PlayableAudioBuffer.FromMonoArray(x, SR) if x.ndim == 1 else PlayableAudioBuffer.FromStereoArrays(x[0], x[1], SR)
    s.Start(when)
    if stop is not None:
        s.Stop(stop)
    return s


def panner(ctx, hrir, A, sr=SR):
    p = SpatialPannerNode(ctx)
    p.HrirAzimuths = A
    p.Hrir = HrirSet.FromArray(hrir, sr)
    return p


def set_params(p, values):
    for name, v in values.items():
        getattr(p, name[0].upper() + name[1:]).Value = float(v)


def render(ctx, frames, pieces=None):
    out = np.zeros((2, frames), np.float32)
    pos = 0
    for k in (pieces or [frames]):
        k = min(k, frames - pos)
        if k > 0:
            ctx.Render(out, k, pos)
            pos += k
    if pos < frames:
        ctx.Render(out, frames - pos, pos)
    return out


def check(out, ref, what):
    scale = max(1.0, float(np.max(np.abs(ref))))
    err = float(np.max(np.abs(out.astype(np.float64) - ref)))
    print(f"{what}: max-abs error {err:.3e} = {err / scale:.3e} x max(1, peak {float(np.max(np.abs(ref))):.3f}); rms {M_rms(out):.3e}")
    assert M_rms(out) > 1e-3          # an all-zero render cannot pass
    assert err <= 1e-5 * scale, (what, err, scale)


def M_rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, np.float64)))))


# ---- 1. delta set: bit for bit --------------------------------------------------------------------------------------------------

DELTA_A, DELTA_E, DELTA_T = 4, 3, 16
CONES = {   # source at (3, 0, 0), listener at the origin: the source-to-listener direction is (-1, 0, 0)
    "off": dict(),
    "inside": dict(orientationX=-1.0, coneInnerAngle=60.0, coneOuterAngle=120.0, coneOuterGain=0.25),                     # angle 0
    "between": dict(orientationX=-1.0, orientationY=1.0, coneInnerAngle=60.0, coneOuterAngle=120.0, coneOuterGain=0.25),  # angle 45
    "outside": dict(orientationX=1.0, coneInnerAngle=60.0, coneOuterAngle=120.0, coneOuterGain=0.25),                     # angle 180
}


def delta_set():
    D = DELTA_A * DELTA_E
    h = np.zeros((D, 2, DELTA_T), np.float32)
    delays = [(3 * d + 1) % DELTA_T for d in range(D)]
    for d in range(D):
        h[d, 0, delays[d]] = 2.0 ** -(d % 3)        # ear gains: powers of two
        h[d, 1, delays[d]] = 2.0 ** -((d + 1) % 4)
    return h, delays


@pytest.mark.parametrize("cone", list(CONES))
@pytest.mark.parametrize("model", [DistanceModelType.Linear, DistanceModelType.Inverse, DistanceModelType.Exponential])
def test_delta_set_bit_for_bit(model, cone):
    frames = 12 * B
    h, delays = delta_set()
    x = G.voice(5, frames)
    x[0] = 1.0                                   # the output at the direction's delay IS the filter tap g x gain
    values = dict(positionX=3.0, refDistance=1.0, maxDistance=10.0, rolloffFactor=0.7, **CONES[cone])   # maxDistance > refDistance
    ctx = OfflineAudioContext(SR)
    s = source(ctx, x)
    p = panner(ctx, h, DELTA_A)
    p.DistanceModel = model
    set_params(p, values)
    s.Connect(p).Connect(ctx.Destination)
    out = render(ctx, frames)
    ctx.Dispose()
    # (3, 0, 0): azimuth +90 = i 1 of 4, elevation 0 = ring 1 of 3: a grid point, weights (1, 0, 0, 0)
    direction, g_test = M.geometry(values, int(model))
    idx, w = M.select(direction, DELTA_A, DELTA_E)
    assert idx[0] == 1 * DELTA_A + 1 and tuple(w) == (1.0, 0.0, 0.0, 0.0)
    d, k = idx[0], delays[idx[0]]
    g_dev = f32(out[0, k] / h[d, 0, k])          # exact: x[0] = 1 and the ear gain is a power of two
    print(f"delta {model.name}/{cone}: device gain {float(g_dev):.9g}, float32 restatement {float(g_test):.9g}")
    assert g_test > 0
    assert abs(float(g_dev) - float(g_test)) <= 1e-6 * float(g_test)
    for ear in range(2):
        want = np.zeros(frames, np.float32)
        want[k:] = f32(g_dev * h[d, ear, k]) * x[:frames - k]      # one float32 product per sample
        assert np.array_equal(out[ear], want), (ear, model, cone)
    assert M_rms(out) > 1e-3


# ---- 2. static source, decaying-noise set ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("stereo", [False, True])
@pytest.mark.parametrize("T", [1, 2, 127, 128, 129, 512])
def test_static_source_against_the_model(T, stereo):
    frames = 12 * B
    A, E = 6, 3
    h = noise_set(A * E, T, 11 + T)
    x = np.stack([G.voice(21, frames), G.voice(22, frames)]) if stereo else G.voice(21, frames)
    for beta in (1.0, 0.3, 0.0):
        values = dict(positionX=1.3, positionY=0.7, positionZ=-2.1, spatialBlend=beta)
        ctx = OfflineAudioContext(SR)
        s = source(ctx, x)
        p = panner(ctx, h, A)
        set_params(p, values)
        s.Connect(p).Connect(ctx.Destination)
        out = render(ctx, frames)
        ctx.Dispose()
        check(out, M.render(x, h, A, values), f"static T={T} stereo={stereo} blend={beta}")


# ---- 3 / 4. moving source ----------------------------------------------------------------------------------------------------------

MOVE_BLOCKS = 20


def stepped_path(nb):
    """one position per block: the azimuth crosses the 360 / 0 seam, the elevation climbs over the pole"""
    pts = []
    for b in range(nb):
        az, el = math.radians(335.0 + 4.0 * b), math.radians(58.0 + 4.0 * b)     # 335 .. 51 degrees ; 58 .. 134 degrees (over +90)
        r = 1.5 + 0.05 * b
        d = (math.sin(az) * math.cos(el), math.sin(el), -math.cos(az) * math.cos(el))
        pts.append(tuple(float(f32(r * c)) for c in (d[0], d[1], -d[2])))        # identity listener: direction z = -(world z)
    return pts


def moving_scene(ctx, x, h, A, kind, bt):
    nb = len(bt) - 1
    s = source(ctx, x)
    p = panner(ctx, h, A)
    if np.ndim(x) == 2:
        p.SpatialBlend.Value = 0.6   # (a stereo fade: both dry gains and both input rows take part)
    if kind == "stepped":
        pts = stepped_path(nb)
        for b, (px, py, pz) in enumerate(pts):
            p.PositionX.SetValueAtTime(px, bt[b])
            p.PositionY.SetValueAtTime(py, bt[b])
            p.PositionZ.SetValueAtTime(pz, bt[b])
        params = [dict(positionX=px, positionY=py, positionZ=pz) for px, py, pz in pts]
        if np.ndim(x) == 2:
            params = [dict(q, spatialBlend=0.6) for q in params]
    else:   # a ramp across the front of the listener
        p.PositionZ.Value = -1.0
        p.PositionY.Value = 0.4
        p.PositionX.SetValueAtTime(-3.0, 0.0)
        p.PositionX.LinearRampToValueAtTime(3.0, bt[nb])
        params = [dict(positionX=M.linear_ramp(-3.0, 0.0, 3.0, bt[nb], bt[b]), positionY=0.4, positionZ=-1.0) for b in range(nb)]
    s.Connect(p).Connect(ctx.Destination)
    return (s, p), params


@pytest.mark.parametrize("kind", ["stepped", "ramp", "ramp_listener"])
def test_moving_source_against_the_model(kind):
    nb, T, A, E = MOVE_BLOCKS, 129, 8, 3
    frames = nb * B
    h = noise_set(A * E, T, 77)
    x = G.voice(31, frames)
    bt = M.block_times(nb, SR)
    ctx = OfflineAudioContext(SR)
    listener = M.IDENTITY
    if kind == "ramp_listener":   # rotated 90 degrees: looking down +x
        ctx.SetListener((0.5, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0))
        listener = M.listener_from((0.5, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    hold, params = moving_scene(ctx, x, h, A, "stepped" if kind == "stepped" else "ramp", bt)
    out = render(ctx, frames)
    ctx.Dispose()
    ref = M.render(x, h, A, params, listener=listener)
    if kind == "ramp_listener":   # the rotation is heard: not the identity listener's output
        assert np.max(np.abs(ref - M.render(x, h, A, params))) > 1e-2
    check(out, ref, f"moving {kind}")


def test_moving_stereo_source_against_the_model():
    """every block fades, with a stereo input and a dry share: the previous block's dry gain and the right input row"""
    nb, T, A, E = MOVE_BLOCKS, 129, 8, 3
    frames = nb * B
    h = noise_set(A * E, T, 78)
    x = np.stack([G.voice(33, frames), G.voice(34, frames)])
    bt = M.block_times(nb, SR)
    outs = []
    for limit in (None, 3):
        ctx = OfflineAudioContext(SR)
        if limit:
            ctx.SetOption("max_chunk_blocks", limit)
        hold, params = moving_scene(ctx, x, h, A, "stepped", bt)
        outs.append(render(ctx, frames))
        ctx.Dispose()
    check(outs[0], M.render(x, h, A, params), "moving stereo")
    assert np.array_equal(outs[0], outs[1])


def test_hrir_set_replaced_between_render_calls():
    """a 24 x 1 set, then a 4-direction set of another length on the same node while the source plays: the first block after the
    change uses its own filters alone (no fade from indices of the set that is gone), the input history carries over"""
    nb, cut = 16, 7
    frames = nb * B
    big, small = noise_set(24, 200, 81), noise_set(4, 129, 82)
    x = G.voice(35, frames)
    bt = M.block_times(nb, SR)
    pts = [(float(f32(2.0 * math.sin(-0.5 - 0.11 * b))), 0.3, float(f32(2.0 * math.cos(-0.5 - 0.11 * b)))) for b in range(nb)]   # azimuths near 330 .. 230: indices 22 .. 15 of 24
    ctx = OfflineAudioContext(SR)
    s = source(ctx, x)
    p = panner(ctx, big, 24)
    for b, (px, py, pz) in enumerate(pts):
        p.PositionX.SetValueAtTime(px, bt[b])
        p.PositionZ.SetValueAtTime(pz, bt[b])
    p.PositionY.Value = 0.3
    s.Connect(p).Connect(ctx.Destination)
    out = np.zeros((2, frames), np.float32)
    ctx.Render(out, cut * B, 0)
    p.Hrir = None                 # (clear first: the new set's channel count does not fit the old azimuth count)
    p.HrirAzimuths = 4
    p.Hrir = HrirSet.FromArray(small, SR)
    ctx.Render(out, frames - cut * B, cut * B)
    ctx.Dispose()
    params = [dict(positionX=px, positionY=py, positionZ=pz) for px, py, pz in pts]
    idx, _ = M.select(M.geometry(params[cut - 1])[0], 24, 1)
    assert max(idx) >= 8          # the block before the change points past the small set's 8 channels
    ref = np.concatenate([M.render(x[:cut * B], big, 24, params[:cut]),
                          M.render(x[cut * B:], small, 4, params[cut:], history=M.mono_mix(x[:cut * B]))], axis=1)
    check(out, ref, "hrir set replaced")


def test_chunking_is_bit_for_bit():
    nb, T, A, E = MOVE_BLOCKS, 129, 8, 3
    frames = nb * B
    h = noise_set(A * E, T, 77)
    x = G.voice(31, frames)
    bt = M.block_times(nb, SR)
    outs = {}
    for name, (limit, pieces) in {"whole": (None, None), "chunks of 5": (5, None), "chunks of 1": (1, None), "two calls": (None, [7 * B])}.items():
        ctx = OfflineAudioContext(SR)
        if limit:
            ctx.SetOption("max_chunk_blocks", limit)
        hold, params = moving_scene(ctx, x, h, A, "stepped", bt)
        outs[name] = render(ctx, frames, pieces)
        ctx.Dispose()
    check(outs["whole"], M.render(x, h, A, params), "chunking, whole")
    for name, o in outs.items():
        assert np.array_equal(o, outs["whole"]), name


# ---- 5. silence -----------------------------------------------------------------------------------------------------------------

def test_silent_input_blocks_are_exact_zeros_and_cut_the_tail():
    nb, T, A, E = 20, 129, 6, 3
    frames = nb * B
    h = noise_set(A * E, T, 91)
    bt = M.block_times(nb, SR)
    a, b2 = G.voice(41, 6 * B), G.voice(42, 6 * B)
    values = dict(positionX=-0.8, positionY=0.3, positionZ=-1.1)
    ctx = OfflineAudioContext(SR)
    s1 = source(ctx, a, bt[3], bt[9])       # blocks 3 .. 8
    s2 = source(ctx, b2, bt[14])            # blocks 14 .. 19
    p = panner(ctx, h, A)
    set_params(p, values)
    s1.Connect(p)
    s2.Connect(p)
    p.Connect(ctx.Destination)
    out = render(ctx, frames)
    ctx.Dispose()
    x = np.zeros(frames, np.float32)
    x[3 * B:9 * B] = a
    x[14 * B:20 * B] = b2
    silent = np.ones(nb, bool)
    silent[3:9] = False
    silent[14:20] = False
    for blk in np.nonzero(silent)[0]:
        assert not out[:, blk * B:(blk + 1) * B].any(), blk     # block 9 holds no filter tail
    check(out, M.render(x, h, A, values, silent=silent), "silence")


def silence_scene(ctx, h, A, bt, moving):
    a, b2 = G.voice(41, 6 * B), G.voice(42, 6 * B)
    s1 = source(ctx, a, bt[3], bt[9])       # blocks 3 .. 8
    s2 = source(ctx, b2, bt[14])            # blocks 14 .. 19
    p = panner(ctx, h, A)
    set_params(p, dict(positionX=-0.8, positionY=0.3, positionZ=-1.1))
    if moving:
        p.PositionX.SetValueAtTime(-0.8, 0.0)
        p.PositionX.LinearRampToValueAtTime(1.7, bt[20])
    s1.Connect(p)
    s2.Connect(p)
    p.Connect(ctx.Destination)
    return (s1, s2, p)


@pytest.mark.parametrize("moving", [False, True])
def test_silence_across_chunk_and_render_call_boundaries(moving):
    """chunks that end inside, on the edge of and right after the silent stretches: the history-only workgroup of a chunk that ends on
    silence, and the previous block's descriptor (dropped by silence, kept otherwise) carried from chunk to chunk"""
    nb, T, A, E = 20, 129, 6, 3
    frames = nb * B
    h = noise_set(A * E, T, 91)
    bt = M.block_times(nb, SR)
    outs = {}
    for name, (limit, pieces) in {"whole": (None, None), "chunks of 1": (1, None), "chunks of 5": (5, None),
                                  "calls": (None, [2 * B, 7 * B, 3 * B, 2 * B])}.items():   # calls end at blocks 2, 9, 12, 14
        ctx = OfflineAudioContext(SR)
        if limit:
            ctx.SetOption("max_chunk_blocks", limit)
        hold = silence_scene(ctx, h, A, bt, moving)
        outs[name] = render(ctx, frames, pieces)
        ctx.Dispose()
    x = np.zeros(frames, np.float32)
    x[3 * B:9 * B] = G.voice(41, 6 * B)
    x[14 * B:20 * B] = G.voice(42, 6 * B)
    silent = np.ones(nb, bool)
    silent[3:9] = False
    silent[14:20] = False
    params = [dict(positionX=M.linear_ramp(-0.8, 0.0, 1.7, bt[20], bt[b]) if moving else -0.8, positionY=0.3, positionZ=-1.1) for b in range(nb)]
    check(outs["whole"], M.render(x, h, A, params, silent=silent), f"silence, moving={moving}")
    for name, o in outs.items():
        assert np.array_equal(o, outs["whole"]), name


# ---- 6. batch -------------------------------------------------------------------------------------------------------------------

def test_batch_of_nodes_sharing_hrir_sets():
    nb = 12
    frames = nb * B
    sets = [(noise_set(6 * 3, 64, 5), 6), (noise_set(4 * 1, 200, 6), 4)]
    ctx = OfflineAudioContext(SR)
    shared = [HrirSet.FromArray(h, SR) for h, _ in sets]
    ref = np.zeros((2, frames))
    hold = []
    bt = M.block_times(nb, SR)
    for v in range(83):
        which = 0 if v < 80 else 1
        h, A = sets[which]
        x = G.voice(100 + v, frames)
        ang = 2.0 * math.pi * v / 83.0
        values = dict(positionX=2.0 * math.sin(ang), positionY=0.5 * math.cos(3 * ang), positionZ=-2.0 * math.cos(ang), spatialBlend=1.0 if v % 4 else 0.6)
        s = source(ctx, x)
        p = SpatialPannerNode(ctx)
        p.HrirAzimuths = A
        p.Hrir = shared[which]
        set_params(p, values)
        params = values
        if v % 10 == 0:   # a few of them move
            p.PositionX.SetValueAtTime(values["positionX"], 0.0)
            p.PositionX.LinearRampToValueAtTime(-values["positionX"] + 0.25, bt[nb])
            params = [dict(values, positionX=M.linear_ramp(values["positionX"], 0.0, -values["positionX"] + 0.25, bt[nb], bt[b])) for b in range(nb)]
        s.Connect(p).Connect(ctx.Destination)
        hold.append((s, p))
        ref += M.render(x, h, A, params)
    out = render(ctx, frames)
    launches = ctx.GetStats()["kernel_launches"]
    ctx.Dispose()
    print("batch: kernel launches", launches)
    assert launches < 40       # one spatial launch for the level, not one per node (83 of them)
    check(out, ref, "batch of 83")


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------

REF_T, REF_A, REF_E = 33, 4, 3


def _refused_then_supported(offend, exc):
    """`offend(ctx, s, p, good)` commits the offence, `offend.undo` takes it back.  A render-time offence raises from Render before
    anything moves; a setter's raises from the setter.  With the offence removed the SAME context renders from time 0, as the model."""
    frames = 12 * B
    h = noise_set(REF_A * REF_E, REF_T, 3)
    x = G.voice(51, frames)
    values = dict(positionX=1.0, positionY=-0.5, positionZ=0.8)
    ctx = OfflineAudioContext(SR)
    s = source(ctx, x)
    p = SpatialPannerNode(ctx)
    set_params(p, values)
    s.Connect(p).Connect(ctx.Destination)

    def good():
        p.HrirAzimuths = REF_A
        p.Hrir = HrirSet.FromArray(h, SR)
    out = np.zeros((2, frames), np.float32)
    with pytest.raises(exc):
        offend(ctx, s, p, good)
        ctx.Render(out, frames, 0)
    assert ctx.CurrentBlock == 0
    offend.undo(ctx, s, p, good)
    ctx.Render(out, frames, 0)
    ctx.Dispose()
    check(out, M.render(x, h, REF_A, values), "after " + offend.__name__)


def _case(undo):
    def deco(fn):
        fn.undo = undo
        return fn
    return deco


@_case(lambda ctx, s, p, good: setattr(p.Occlusion, "Value", 0.0))
def occlusion(ctx, s, p, good):
    good()
    p.Occlusion.Value = 0.5


_consts = {}


def _disconnect_const(ctx, s, p, good):
    _consts.pop(id(ctx)).Disconnect(p.PositionX)


@_case(_disconnect_const)
def signal_on_position(ctx, s, p, good):
    good()
    c = ConstantSourceNode(ctx)
    c.Offset.Value = 0.5
    c.Connect(p.PositionX)
    c.Start()
    _consts[id(ctx)] = c


@_case(lambda ctx, s, p, good: good())
def no_hrir_set(ctx, s, p, good):
    pass


@_case(lambda ctx, s, p, good: good())
def set_of_513_taps(ctx, s, p, good):
    p.HrirAzimuths = REF_A
    p.Hrir = HrirSet.FromArray(noise_set(REF_A * REF_E, 513, 4), SR)


@_case(lambda ctx, s, p, good: good())
def channels_no_multiple_of_azimuths(ctx, s, p, good):
    p.HrirAzimuths = REF_A
    p.Hrir = HrirSet.FromArray(noise_set(REF_A * REF_E + 1, REF_T, 4), SR)     # 2 D = 26, 2 A = 8


@_case(lambda ctx, s, p, good: good())
def sample_rate_mismatch(ctx, s, p, good):
    p.HrirAzimuths = REF_A
    p.Hrir = HrirSet.FromArray(noise_set(REF_A * REF_E, REF_T, 4), 44100)


@pytest.mark.parametrize("offend,exc", [(occlusion, NotSupportedException), (signal_on_position, NotSupportedException),
                                        (no_hrir_set, NotSupportedException), (set_of_513_taps, InvalidOperationException),
                                        (channels_no_multiple_of_azimuths, InvalidOperationException),
                                        (sample_rate_mismatch, InvalidOperationException)],
                         ids=lambda v: getattr(v, "__name__", None))
def test_refusals(offend, exc):
    _refused_then_supported(offend, exc)


def test_pseudo_parameters_take_values_only():
    from graphaudio_amd import ArgumentException
    ctx = OfflineAudioContext(SR)
    p = SpatialPannerNode(ctx)
    assert p.DistanceModel == DistanceModelType.Inverse and p.HrirAzimuths == 1
    for index in (17, 18):
        with pytest.raises(ArgumentException):
            ctx._call("param_set_value_at_time", p._id, index, 1.0, 0.0)
        with pytest.raises(ArgumentException):
            ctx._call("param_linear_ramp_to_value_at_time", p._id, index, 1.0, 1.0)
        with pytest.raises(ArgumentException):
            ctx._call("param_set_target_at_time", p._id, index, 1.0, 0.0, 0.1)
        c = ConstantSourceNode(ctx)
        with pytest.raises(ArgumentException):
            ctx._call("node_connect_param", c._id, p._id, index, 0)
    p.DistanceModel = DistanceModelType.Exponential
    import ctypes as C
    v = C.c_float(-1)
    ctx._call("param_get_value", p._id, 17, C.byref(v))
    assert v.value == 2.0
    p.HrirAzimuths = 24
    ctx._call("param_get_value", p._id, 18, C.byref(v))
    assert v.value == 24.0
    assert [round(q.Value, 3) for q in p._params] == [round(d, 3) for _, d, _, _ in SpatialPannerNode.PARAMS]
    ctx.Dispose()
