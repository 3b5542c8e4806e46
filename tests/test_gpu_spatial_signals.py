"""SpatialPannerNode parameters driven by signals (option "spatial_param_signals"; DESIGN.md "SpatialPannerNode", "Parameters driven
by signals") against the float64 model of tests/_spatial_model.py, one parameter dict per block.

The value of a modulated parameter in block b is clamp(f32(intrinsic + mod[b])), where mod[b] is sample b * 128 of the modulator
sub-graph rendered alone on the device and the intrinsic value is the timeline's (or Value).  Bound: the existing one of
tests/test_gpu_spatial.py, max-abs <= 1e-5 x max(1, peak of the model's output).  Every scene asserts on the CPU that no processed
block sits where the definition jumps: a directivity within 1e-4 of the 0.999 switch, or a distance below 0.01.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from graphaudio_amd import (ChannelCountMode, ConstantSourceNode, DelayNode, DistanceModelType, GainNode, HrirSet, NotSupportedException,
                            OfflineAudioContext, OscillatorNode, OscillatorType, SpatialPannerNode)
from tests import _graphs as G
from tests import _spatial_model as M
from tests.test_gpu_spatial import M_rms, check, noise_set, panner, render, set_params, source

SR = 48000
B = 128
f32 = np.float32
RANGES = {name: (mn, mx) for name, _, mn, mx in SpatialPannerNode.PARAMS}


def new_context(option=1, **opts):
    ctx = OfflineAudioContext(SR)
    if option is not None:
        ctx.SetOption("spatial_param_signals", option)
    for k, v in opts.items():
        ctx.SetOption(k, v)
    return ctx


def attr(p, name):
    return getattr(p, name[0].upper() + name[1:])


def mod_values(build, nb):
    """sample b * 128 of the modulator sub-graph `build(ctx)` rendered alone on the device, b < nb -- into a destination of one channel,
    explicit, which mixes what is connected to it as an AudioParam's modulation input does (AudioParam.cs:68,97-101: a GainNode's
    stereo output arrives as (L + R) / sqrt(2))"""
    ctx = OfflineAudioContext(SR)
    ctx.Destination.SetChannelCount(1)
    ctx.Destination.Inputs[0].SetChannelCountMode(ChannelCountMode.Explicit)
    node = build(ctx)
    node.Connect(ctx.Destination)
    out = np.zeros((1, nb * B), np.float32)
    ctx.Render(out, nb * B, 0)
    ctx.Dispose()
    return out[0, ::B].copy()


def modulated(name, intrinsic, mod):
    """AudioParam.ComputeKRate: Math.Clamp(intrinsicValue + modulation, min, max) in float32"""
    mn, mx = (f32(v) for v in RANGES[name])
    return float(M._clamp(f32(f32(intrinsic) + f32(mod)), mn, mx))


def directivity_and_distance(p, listener=M.IDENTITY):
    """the two quantities of the model's geometry (M.geometry, the same float32 statements) at which the definition jumps"""
    q = {k: f32(v) for k, v in M.PARAM_DEFAULTS.items()}
    q.update({k: f32(v) for k, v in p.items()})
    origin = tuple(f32(c) for c in listener[0])
    w = [f32(q["positionX"] - origin[0]), f32(q["positionY"] - origin[1]), f32(q["positionZ"] - origin[2])]
    distance = f32(np.sqrt(M._dot3(w, w)))
    if distance > f32(0.0001):
        w = [f32(c * f32(f32(1.0) / distance)) for c in w]
    directivity = f32(1.0)
    inner, outer, outer_gain = q["coneInnerAngle"], q["coneOuterAngle"], q["coneOuterGain"]
    if inner < f32(360) or outer < f32(360):
        ori = (q["orientationX"], q["orientationY"], q["orientationZ"])
        mag = f32(np.sqrt(M._dot3(ori, ori)))
        if mag > f32(0.0001):
            n = [f32(c * f32(f32(1.0) / mag)) for c in ori]
            dot = M._clamp(M._dot3(n, [f32(-c) for c in w]), f32(-1), f32(1))
            a = abs(f32(f32(f32(np.arccos(dot)) * f32(180.0)) / f32(math.pi)))
            hi_, ho = f32(inner * f32(0.5)), f32(outer * f32(0.5))
            if a >= ho:
                directivity = outer_gain
            elif a > hi_:
                directivity = f32(f32(1.0) + f32(f32(f32(a - hi_) / f32(ho - hi_)) * f32(outer_gain - f32(1.0))))
    return float(directivity), float(distance)


def guard(params, nb, silent=None, listener=M.IDENTITY, model=M.INVERSE):
    """no processed block where the definition jumps (a scene that fails here has to be changed)"""
    params = [params] * nb if isinstance(params, dict) else params
    for b in range(nb):
        if silent is not None and silent[b]:
            continue
        directivity, distance = directivity_and_distance(params[b], listener)
        # (the restatement above is held to the model: the model's own gain is its gain without the cone times this directivity)
        if model is not None:
            _, g = M.geometry(params[b], model, listener)
            _, g_open = M.geometry(dict(params[b], coneInnerAngle=360.0, coneOuterAngle=360.0), model, listener)
            assert g == f32(g_open * (f32(directivity) if directivity < 0.999 else f32(1.0))), (b, directivity, g, g_open)
        assert abs(directivity - 0.999) > 1e-4, (b, directivity)
        assert distance >= 0.01, (b, distance)


def const(ctx, value, when=None, stop=None):
    c = ConstantSourceNode(ctx)
    c.Offset.Value = float(value)
    c.Start(*([] if when is None else [when]))
    if stop is not None:
        c.Stop(stop)
    return c


# ---- 1. the graph the option-off refusal test pins ---------------------------------------------------------------------------------

def test_constant_signal_on_position_x():
    """tests/test_gpu_spatial.py::test_refusals[signal_on_position]'s graph with the option on: renders, and is the model at 1.5"""
    frames = 12 * B
    h = noise_set(12, 33, 3)
    x = G.voice(51, frames)
    values = dict(positionX=1.0, positionY=-0.5, positionZ=0.8)
    ctx = new_context()
    s = source(ctx, x)
    p = panner(ctx, h, 4)
    set_params(p, values)
    s.Connect(p).Connect(ctx.Destination)
    c = const(ctx, 0.5)
    c.Connect(p.PositionX)
    out = render(ctx, frames)
    ctx.Dispose()
    want = dict(values, positionX=modulated("positionX", 1.0, 0.5))
    assert want["positionX"] == 1.5
    guard(want, 12)
    ref = M.render(x, h, 4, want)
    assert np.max(np.abs(ref - M.render(x, h, 4, values))) > 1e-2      # the signal is heard
    check(out, ref, "constant signal on positionX")


# ---- 2. constant signals on the other parameters, every distance model -------------------------------------------------------------

@pytest.mark.parametrize("model", [DistanceModelType.Linear, DistanceModelType.Inverse, DistanceModelType.Exponential])
def test_constant_signals_on_many_parameters(model):
    frames = 10 * B
    h = noise_set(12, 33, 5)
    x = G.voice(52, frames)
    intrinsic = dict(positionX=2.0, positionY=-0.5, positionZ=0.8, orientationX=-0.2, orientationY=0.1, orientationZ=0.3, refDistance=0.5,
                     maxDistance=12.0, rolloffFactor=0.4, coneInnerAngle=60.0, coneOuterAngle=170.0, coneOuterGain=0.2, spatialBlend=0.8)
    signals = dict(positionY=1.25, positionZ=-2.0, orientationX=-1.5, orientationY=0.8, orientationZ=0.3, refDistance=0.75,
                   rolloffFactor=0.5, spatialBlend=0.5, coneOuterGain=-0.5)
    ctx = new_context()
    s = source(ctx, x)
    p = panner(ctx, h, 4)
    p.DistanceModel = model
    set_params(p, intrinsic)
    s.Connect(p).Connect(ctx.Destination)
    hold = []
    for name, v in signals.items():
        c = const(ctx, v)
        c.Connect(attr(p, name))
        hold.append(c)
    out = render(ctx, frames)
    ctx.Dispose()
    want = dict(intrinsic)
    for name, v in signals.items():
        want[name] = modulated(name, intrinsic[name], v)
    assert want["spatialBlend"] == 1.0 and want["coneOuterGain"] == 0.0 and want["orientationX"] == -1.0     # clamped
    guard(want, 10, model=int(model))
    directivity, _ = directivity_and_distance(want)
    assert 0.05 < directivity < 0.95                                   # between the cone's angles
    ref = M.render(x, h, 4, want, model=int(model))
    assert np.max(np.abs(ref - M.render(x, h, 4, intrinsic, model=int(model)))) > 1e-2
    check(out, ref, f"constant signals, {model.name}")


# ---- 3. moving source ----------------------------------------------------------------------------------------------------------------

MOVE_BLOCKS, MOVE_T, MOVE_A, MOVE_E = 300, 129, 8, 3
_cache = {}


def move_modulators(nb):
    bt = M.block_times(nb, SR)

    def sine(ctx):
        o = OscillatorNode(ctx)
        o.Frequency.Value = 2.5
        g = GainNode(ctx)
        g.Gain.Value = 1.5
        o.Connect(g)
        o.Start()
        return g

    def triangle(ctx):
        o = OscillatorNode(ctx)
        o.Type = OscillatorType.Triangle
        o.Frequency.Value = 1.7
        o.Start()
        return o

    def ramped(ctx):
        c = ConstantSourceNode(ctx)
        c.Offset.SetValueAtTime(0.25, 0.0)
        c.Offset.LinearRampToValueAtTime(-0.6, bt[nb])
        c.Start()
        return c

    return dict(positionX=sine, positionZ=triangle, positionY=ramped)


def move_scene(ctx, x, h, nb, extra=None):
    """a source that swings across the front of the listener: every block's descriptor differs from the one before"""
    bt = M.block_times(nb, SR)
    s = source(ctx, x)
    p = panner(ctx, h, MOVE_A)
    set_params(p, dict(positionX=0.3, positionZ=-2.0))
    if np.ndim(x) == 2:
        p.SpatialBlend.Value = 0.6
    p.PositionY.SetValueAtTime(-0.5, 0.0)
    p.PositionY.LinearRampToValueAtTime(0.7, bt[nb])
    s.Connect(p).Connect(ctx.Destination)
    hold = [s, p]
    for name, build in move_modulators(nb).items():
        m = build(ctx)
        m.Connect(attr(p, name))
        hold.append(m)
    if extra:
        hold.append(extra(ctx, s, p))
    return hold


def move_params(nb, stereo):
    key = ("params", nb, stereo)
    if key not in _cache:
        bt = M.block_times(nb, SR)
        mods = {name: mod_values(build, nb) for name, build in move_modulators(nb).items()}
        params = []
        for b in range(nb):
            q = dict(positionX=modulated("positionX", 0.3, mods["positionX"][b]), positionZ=modulated("positionZ", -2.0, mods["positionZ"][b]),
                     positionY=modulated("positionY", M.linear_ramp(-0.5, 0.0, 0.7, bt[nb], bt[b]), mods["positionY"][b]))
            if stereo:
                q["spatialBlend"] = 0.6
            params.append(q)
        if nb == MOVE_BLOCKS:       # the whole swing: more than one period of both oscillators
            assert np.ptp(mods["positionX"]) > 2.0 and np.ptp(mods["positionZ"]) > 1.5 and np.ptp(mods["positionY"]) > 0.5
        guard(params, nb)
        _cache[key] = params
    return _cache[key]


def move_input(nb, stereo):
    frames = nb * B
    return np.stack([G.voice(33, frames), G.voice(34, frames)]) if stereo else G.voice(31, frames)


def move_reference(nb, stereo):
    key = ("ref", nb, stereo)
    if key not in _cache:
        h = noise_set(MOVE_A * MOVE_E, MOVE_T, 77)
        ref = M.render(move_input(nb, stereo), h, MOVE_A, move_params(nb, stereo))
        ref.setflags(write=False)
        _cache[key] = ref
    return _cache[key]


def move_render(nb, stereo=False, pieces=None, extra=None, **opts):
    h = noise_set(MOVE_A * MOVE_E, MOVE_T, 77)
    ctx = new_context(**opts)
    hold = move_scene(ctx, move_input(nb, stereo), h, nb, extra)
    out = render(ctx, nb * B, pieces)
    ctx.Dispose()
    return out


@pytest.mark.parametrize("stereo", [False, True])
def test_moving_source_driven_by_oscillators(stereo):
    """300 blocks (several waves of lanes): a sine through a depth gain on positionX, a triangle on positionZ, positionY on a
    linear-ramp timeline plus a ConstantSource whose Offset ramps"""
    out = move_render(MOVE_BLOCKS, stereo)
    check(out, move_reference(MOVE_BLOCKS, stereo), f"moving, stereo={stereo}")


# ---- 4. a modulator that is silent in part -----------------------------------------------------------------------------------------

def test_modulator_silent_in_part():
    nb = 20
    frames = nb * B
    bt = M.block_times(nb, SR)
    h = noise_set(12, 33, 7)
    x = G.voice(53, frames)
    values = dict(positionX=1.0, positionY=0.4, positionZ=-1.2)
    when, stop = bt[7], bt[13] + 50.0 / SR
    ctx = new_context()
    s = source(ctx, x)
    p = panner(ctx, h, 4)
    set_params(p, values)
    s.Connect(p).Connect(ctx.Destination)
    c = const(ctx, 0.8, when, stop)
    c.Connect(p.PositionX)
    out = render(ctx, frames)
    ctx.Dispose()
    mod = mod_values(lambda cx: const(cx, 0.8, when, stop), nb)
    assert not mod[:7].any() and not mod[14:].any() and mod[7] == f32(0.8) and mod[13] == f32(0.8)   # starts with block 7, stops inside block 13
    params = [dict(values, positionX=modulated("positionX", 1.0, mod[b])) for b in range(nb)]
    guard(params, nb)
    assert params[6]["positionX"] == 1.0 and params[7]["positionX"] == float(f32(1.8)) and params[14]["positionX"] == 1.0
    ref = M.render(x, h, 4, params)
    still = M.render(x, h, 4, [params[7]] * nb)
    assert np.max(np.abs(ref[:, 7 * B:8 * B] - still[:, 7 * B:8 * B])) > 1e-2      # block 7 fades
    check(out, ref, "modulator silent in part")


# ---- 5. chunking ---------------------------------------------------------------------------------------------------------------------

def test_chunking_is_bit_for_bit():
    nb = MOVE_BLOCKS
    whole = move_render(nb)
    check(whole, move_reference(nb, False), "chunking, whole")
    for k in (1, 5, 7):
        assert np.array_equal(move_render(nb, pieces=[k * B] * (nb // k + 1)), whole), f"render calls of {k} blocks"
    assert np.array_equal(move_render(nb, max_chunk_blocks=4), whole), "max_chunk_blocks 4"


# ---- 6. silence ------------------------------------------------------------------------------------------------------------------------

def test_silent_input_blocks_under_a_modulated_position():
    nb, T, A, E = 20, 129, 6, 3
    frames = nb * B
    h = noise_set(A * E, T, 91)
    bt = M.block_times(nb, SR)
    a, b2 = G.voice(41, 6 * B), G.voice(42, 6 * B)

    def lfo(ctx):
        o = OscillatorNode(ctx)
        o.Frequency.Value = 11.0
        o.Start()
        return o

    outs = {}
    for name, (limit, pieces) in {"whole": (None, None), "chunks of 1": (1, None), "chunks of 5": (5, None),
                                  "calls": (None, [2 * B, 7 * B, 3 * B, 2 * B])}.items():   # calls end at blocks 2, 9, 12, 14
        ctx = new_context(**({"max_chunk_blocks": limit} if limit else {}))
        s1 = source(ctx, a, bt[3], bt[9])       # blocks 3 .. 8
        s2 = source(ctx, b2, bt[14])            # blocks 14 .. 19
        p = panner(ctx, h, A)
        set_params(p, dict(positionX=-0.8, positionY=0.3, positionZ=-1.1))
        s1.Connect(p)
        s2.Connect(p)
        p.Connect(ctx.Destination)
        m = lfo(ctx)
        m.Connect(p.PositionX)
        outs[name] = render(ctx, frames, pieces)
        ctx.Dispose()
    x = np.zeros(frames, np.float32)
    x[3 * B:9 * B] = a
    x[14 * B:20 * B] = b2
    silent = np.ones(nb, bool)
    silent[3:9] = False
    silent[14:20] = False
    mod = mod_values(lfo, nb)
    params = [dict(positionX=modulated("positionX", -0.8, mod[b]), positionY=0.3, positionZ=-1.1) for b in range(nb)]
    guard(params, nb, silent)
    for blk in np.nonzero(silent)[0]:
        assert not outs["whole"][:, blk * B:(blk + 1) * B].any(), blk     # exact zeros; block 9 holds no filter tail
    # (the model's block 14 uses its own filters alone -- no fade in the first block after silence -- although its position differs from block 8's)
    assert params[14]["positionX"] != params[8]["positionX"]
    check(outs["whole"], M.render(x, h, A, params, silent=silent), "silence under a modulated position")
    for name, o in outs.items():
        assert np.array_equal(o, outs["whole"]), name


# ---- 7. transitions between render calls ---------------------------------------------------------------------------------------------

def test_connect_and_disconnect_between_render_calls():
    """10 blocks on the host's descriptors, 10 on the device's, 10 on the host's again: the first block of each part fades from
    the descriptor the other side made"""
    nb = 30
    frames = nb * B
    h = noise_set(12, 65, 9)
    x = G.voice(54, frames)
    values = dict(positionX=1.0, positionY=-0.5, positionZ=0.8)
    ctx = new_context()
    s = source(ctx, x)
    p = panner(ctx, h, 4)
    set_params(p, values)
    s.Connect(p).Connect(ctx.Destination)
    out = np.zeros((2, frames), np.float32)
    ctx.Render(out, 10 * B, 0)
    c = const(ctx, 0.6)
    c.Connect(p.PositionX)
    ctx.Render(out, 10 * B, 10 * B)
    c.Disconnect(p.PositionX)
    p.PositionX.Value = 1.6       # continues where the signal left it ...
    p.PositionY.Value = 0.9       # ... and moves up: block 20 fades from the descriptor the device made
    ctx.Render(out, 10 * B, 20 * B)
    ctx.Dispose()
    mid = dict(values, positionX=modulated("positionX", 1.0, 0.6))
    last = dict(mid, positionY=0.9)
    assert mid["positionX"] == float(f32(1.6))
    params = [values] * 10 + [mid] * 10 + [last] * 10
    guard(params, nb)
    ref = M.render(x, h, 4, params)
    for join, after in ((10, mid), (20, last)):       # both joins fade audibly
        alone = M.render(x, h, 4, [after] * nb)
        assert np.max(np.abs(ref[:, join * B:(join + 1) * B] - alone[:, join * B:(join + 1) * B])) > 1e-2
    check(out, ref, "connect / disconnect between render calls")


# ---- 8. a new HRIR set while signal-driven -----------------------------------------------------------------------------------------------

def test_hrir_set_replaced_while_signal_driven():
    nb, cut = 16, 7
    frames = nb * B
    big, small = noise_set(24, 200, 81), noise_set(4, 129, 82)
    x = G.voice(35, frames)

    def lfo(ctx):
        o = OscillatorNode(ctx)
        o.Frequency.Value = 9.0
        g = GainNode(ctx)
        g.Gain.Value = 2.0
        o.Connect(g)
        o.Start()
        return g

    ctx = new_context()
    s = source(ctx, x)
    p = panner(ctx, big, 24)
    set_params(p, dict(positionX=-3.0, positionY=0.3, positionZ=1.5))      # to the left of the listener: azimuths past 180 degrees
    s.Connect(p).Connect(ctx.Destination)
    m = lfo(ctx)
    m.Connect(p.PositionX)
    out = np.zeros((2, frames), np.float32)
    ctx.Render(out, cut * B, 0)
    p.Hrir = None
    p.HrirAzimuths = 4
    p.Hrir = HrirSet.FromArray(small, SR)
    ctx.Render(out, frames - cut * B, cut * B)
    ctx.Dispose()
    mod = mod_values(lfo, nb)
    params = [dict(positionX=modulated("positionX", -3.0, mod[b]), positionY=0.3, positionZ=1.5) for b in range(nb)]
    guard(params, nb)
    idx, _ = M.select(M.geometry(params[cut - 1])[0], 24, 1)
    assert max(idx) >= 8          # the block before the change points past the small set's 8 channels
    ref = np.concatenate([M.render(x[:cut * B], big, 24, params[:cut]),
                          M.render(x[cut * B:], small, 4, params[cut:], history=M.mono_mix(x[:cut * B]))], axis=1)
    check(out, ref, "hrir set replaced while signal-driven")


# ---- 9. signal-driven, timeline-driven and static nodes in one level ---------------------------------------------------------------------

def _mixed_scene(ctx, nb, signals):
    frames = nb * B
    sets = [(noise_set(6 * 3, 64, 5), 6), (noise_set(4 * 1, 200, 6), 4)]
    shared = [HrirSet.FromArray(h, SR) for h, _ in sets]
    bt = M.block_times(nb, SR)
    hold, scene = [], []
    for v in range(70):
        which = 0 if v % 7 else 1
        h, A = sets[which]
        x = G.voice(300 + v, frames)
        ang = 2.0 * math.pi * v / 70.0
        values = dict(positionX=2.0 * math.sin(ang), positionY=0.5 * math.cos(3 * ang), positionZ=-2.0 * math.cos(ang), spatialBlend=1.0 if v % 4 else 0.6)
        s = source(ctx, x)
        p = SpatialPannerNode(ctx)
        p.HrirAzimuths = A
        p.Hrir = shared[which]
        set_params(p, values)
        kind = ("signal", "timeline", "static")[v % 3]
        build = None
        if kind == "timeline":
            p.PositionX.SetValueAtTime(values["positionX"], 0.0)
            p.PositionX.LinearRampToValueAtTime(-values["positionX"] + 0.25, bt[nb])
        if kind == "signal":
            def build(cx, v=v):
                o = OscillatorNode(cx)
                o.Type = OscillatorType.Triangle if v % 2 else OscillatorType.Sine
                o.Frequency.Value = 3.0 + 0.37 * v
                g = GainNode(cx)
                g.Gain.Value = 0.5 + 0.01 * v
                o.Connect(g)
                o.Start()
                return g
            if signals:
                m = build(ctx)
                m.Connect(p.PositionZ if v % 2 else p.PositionX)
                hold.append(m)
        s.Connect(p).Connect(ctx.Destination)
        hold.append((s, p))
        scene.append((x, h, A, values, kind, build, "positionZ" if v % 2 else "positionX"))
    return hold, scene


def test_mixed_nodes_in_one_level():
    nb = 12
    frames = nb * B
    bt = M.block_times(nb, SR)
    ctx = new_context()
    hold, scene = _mixed_scene(ctx, nb, True)
    out = render(ctx, frames)
    launches = ctx.GetStats()["kernel_launches"]
    ctx.Dispose()
    print("mixed: kernel launches", launches)
    assert launches < 40       # one descriptor launch and one panner launch for the level, not one per node
    ref = np.zeros((2, frames))
    kinds = {"signal": 0, "timeline": 0, "static": 0}
    for x, h, A, values, kind, build, name in scene:
        params = values
        if kind == "timeline":
            params = [dict(values, positionX=M.linear_ramp(values["positionX"], 0.0, -values["positionX"] + 0.25, bt[nb], bt[b])) for b in range(nb)]
        if kind == "signal":
            mod = mod_values(build, nb)
            params = [dict(values, **{name: modulated(name, values[name], mod[b])}) for b in range(nb)]
        guard(params, nb)
        kinds[kind] += 1
        ref += M.render(x, h, A, params)
    assert min(kinds.values()) >= 23
    check(out, ref, "mixed level of 70")


def test_option_without_signals_changes_nothing():
    nb = 12
    outs = []
    for option in (0, 1):
        ctx = new_context(option)
        hold, _ = _mixed_scene(ctx, nb, False)
        outs.append(render(ctx, nb * B))
        ctx.Dispose()
    assert M_rms(outs[0]) > 1e-3
    assert np.array_equal(outs[0], outs[1])


# ---- 10. occlusion and transmission ------------------------------------------------------------------------------------------------

def test_signal_on_occlusion_is_refused_and_transmission_has_no_effect():
    frames = 12 * B
    h = noise_set(12, 33, 3)
    x = G.voice(51, frames)
    values = dict(positionX=1.0, positionY=-0.5, positionZ=0.8)
    ctx = new_context()
    s = source(ctx, x)
    p = panner(ctx, h, 4)
    set_params(p, values)
    s.Connect(p).Connect(ctx.Destination)
    c = const(ctx, 0.0)
    c.Connect(p.Occlusion)
    out = np.zeros((2, frames), np.float32)
    with pytest.raises(NotSupportedException, match="occlusion"):
        ctx.Render(out, frames, 0)
    assert ctx.CurrentBlock == 0
    c.Disconnect(p.Occlusion)
    t = const(ctx, 0.7)
    t.Connect(p.TransmissionLow)
    ctx.Render(out, frames, 0)
    ctx.Dispose()
    guard(values, 12)
    check(out, M.render(x, h, 4, values), "signal on transmissionLow")


# ---- 11. feedback ----------------------------------------------------------------------------------------------------------------------

def _feedback_branch(ctx, s, p):
    """source -> delay <-> gain 0.5 (a loop), heard through a gain of 0"""
    d = DelayNode(ctx, 0.1)
    d.DelayTime.Value = 0.01
    fb = GainNode(ctx)
    fb.Gain.Value = 0.5
    mute = GainNode(ctx)
    mute.Gain.Value = 0.0
    s.Connect(d)
    d.Connect(fb)
    fb.Connect(d)
    d.Connect(mute)
    mute.Connect(ctx.Destination)
    return (d, fb, mute)


def test_feedback_loop_elsewhere_in_the_graph():
    nb = 40
    plain = move_render(nb)
    check(plain, move_reference(nb, False), "40 blocks without the loop")
    looped = move_render(nb, extra=_feedback_branch, cycle_delay_split=0)       # one block per chunk
    assert np.array_equal(looped, plain)


def test_feedback_through_a_parameter_renders():
    """the panner's own output, scaled, on its positionX: the loop closes through the block the panner put out last (the existing cycle
    machinery, one block per chunk).  Block b's modulation is sample 0 of block b - 1 of the render itself, mixed down to mono
    ((L + R) / sqrt(2), AudioNodeInput.cs:214-228) behind the gain."""
    nb = 24
    frames = nb * B
    h = noise_set(12, 33, 13)
    x = G.voice(55, frames)
    values = dict(positionX=0.5, positionY=0.2, positionZ=-1.5)
    depth = 4.0
    ctx = new_context()
    s = source(ctx, x)
    p = panner(ctx, h, 4)
    set_params(p, values)
    s.Connect(p).Connect(ctx.Destination)
    g = GainNode(ctx)
    g.Gain.Value = depth
    p.Connect(g)
    g.Connect(p.PositionX)
    out = render(ctx, frames)
    ctx.Dispose()
    params, mods = [], []
    for b in range(nb):
        prev = out[:, (b - 1) * B] if b else np.zeros(2, np.float32)
        mod = f32(f32(f32(prev[0] * f32(depth)) + f32(prev[1] * f32(depth))) * f32(1.0 / math.sqrt(2.0)))
        mods.append(float(mod))
        params.append(dict(values, positionX=modulated("positionX", 0.5, mod)))
    guard(params, nb)
    assert np.ptp(mods) > 0.2                    # the loop moves the source
    check(out, M.render(x, h, 4, params), "feedback through positionX")
