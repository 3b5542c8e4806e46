"""SpatialPannerNode occlusion and three-band transmission on the device (option "spatial_occlusion"; DESIGN.md "SpatialPannerNode",
"Occlusion and transmission") against the float64 model of tests/_spatial_direct_model.py, one parameter dict per block.

Bound: the node's existing one, max-abs <= 1e-5 x max(1, peak of the model's output) (tests/test_gpu_spatial.py); chunkings and render
calls are bit for bit.  Measured on an MI355X (printed by every case): at most 6.7e-7 x that scale (T = 512, the binaural stage's own
figure), at most 1.4e-7 with T = 33, 4.1e-7 x the sum's peak for 70 nodes.  No scene puts a processed block where the definition jumps: positions and cones are those of the existing
tests' guarded scenes, and no block has occlusion = 1 with all three transmissions 0 (s = 0).
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from graphaudio_amd import GainNode, HrirSet, NotSupportedException, OfflineAudioContext, OscillatorNode, SpatialPannerNode
from tests import _graphs as G
from tests import _spatial_direct_model as DM
from tests import _spatial_model as M
from tests.test_gpu_spatial import M_rms, check, noise_set, panner, render, set_params, source
from tests.test_gpu_spatial_signals import const, guard, mod_values, modulated

SR = 48000
B = 128
f32 = np.float32
POSITION = dict(positionX=1.0, positionY=-0.5, positionZ=0.8)
WALL = dict(occlusion=1.0, transmissionLow=0.9, transmissionMid=0.5, transmissionHigh=0.1)
GEOMETRY = set(M.PARAM_DEFAULTS)


def new_context(occlusion=1, **opts):
    ctx = OfflineAudioContext(SR)
    if occlusion is not None:
        ctx.SetOption("spatial_occlusion", occlusion)
    for k, v in opts.items():
        ctx.SetOption(k, v)
    return ctx


def attr(p, name):
    return getattr(p, name[0].upper() + name[1:])


def guarded(params, nb, silent=None):
    params = [params] * nb if isinstance(params, dict) else params
    guard([{k: v for k, v in q.items() if k in GEOMETRY} for q in params], nb, silent)
    for q in params:
        assert DM.block_occlusion(q)[0] > 0
    return params


def hrir_set(T=33):
    return noise_set(12, T, 3)


# ---- 1. frequency-independent occlusion; occlusion 0 under the option ---------------------------------------------------------------

def test_occlusion_without_transmission():
    """all transmissions 0: 1 - occlusion in every band, a plain gain -- no band filter runs, the EQ triple stays the identity"""
    frames = 12 * B
    h, x = hrir_set(), G.voice(51, frames)
    values = dict(POSITION, occlusion=0.6)
    ctx = new_context()
    s = source(ctx, x)
    p = panner(ctx, h, 4)
    set_params(p, values)
    s.Connect(p).Connect(ctx.Destination)
    out = render(ctx, frames)
    ctx.Dispose()
    guarded(values, 12)
    s_, triple = DM.block_occlusion(values)
    assert s_ == f32(f32(1) - f32(0.6)) and triple == DM.EQ_IDENTITY
    ref = DM.render(x, h, 4, values)
    assert np.max(np.abs(ref - M.render(x, h, 4, POSITION))) > 1e-2      # the occlusion is heard
    check(out, ref, "occlusion 0.6, no transmission")


def test_occlusion_zero_is_the_render_without_the_option():
    """transmission set, occlusion 0 throughout: with the option on the output is the option-off output bit for bit"""
    frames = 12 * B
    h, x = noise_set(12, 129, 3), np.stack([G.voice(51, frames), G.voice(52, frames)])
    values = dict(POSITION, spatialBlend=0.5, occlusion=0.0, transmissionLow=0.9, transmissionMid=0.5, transmissionHigh=0.1)
    outs = []
    for option in (None, 0, 1):
        ctx = new_context(option)
        s = source(ctx, x)
        p = panner(ctx, h, 4)
        set_params(p, values)
        s.Connect(p).Connect(ctx.Destination)
        outs.append(render(ctx, frames))
        ctx.Dispose()
    assert M_rms(outs[0]) > 1e-3
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


# ---- 2. a wall: constant occlusion 1 with three different transmissions ----------------------------------------------------------------

@pytest.mark.parametrize("stereo,T", [(False, 33), (True, 33), (False, 512)], ids=["mono", "stereo_blend_0.5", "mono_512_taps"])
def test_constant_wall(stereo, T):
    nb = 16
    frames = nb * B
    h = hrir_set(T)
    x = np.stack([G.voice(61, frames), G.voice(62, frames)]) if stereo else G.voice(61, frames)
    values = dict(POSITION, **WALL)
    if stereo:
        values["spatialBlend"] = 0.5       # the dry path carries the EQ
    ctx = new_context()
    s = source(ctx, x)
    p = panner(ctx, h, 4)
    set_params(p, values)
    s.Connect(p).Connect(ctx.Destination)
    out = render(ctx, frames)
    ctx.Dispose()
    guarded(values, nb)
    s_, triple = DM.block_occlusion(values)
    assert s_ == f32(0.9) and triple != DM.EQ_IDENTITY
    ref = DM.render(x, h, 4, values)
    plain = M.render(x, h, 4, dict({k: v for k, v in values.items() if k in GEOMETRY}))
    assert np.max(np.abs(ref - float(s_) * plain)) > 1e-2      # more than the plain gain: the EQ is heard
    check(out, ref, f"wall, stereo={stereo}, T={T}")


# ---- 3. a timeline: 0 -> 1 -> 0 -> 0.7 -> 0 with steps of the transmissions ---------------------------------------------------------

TL_BLOCKS = 24


def timeline_values(nb=TL_BLOCKS):
    occ = [0.0] * 4 + [1.0] * 6 + [0.0] * 4 + [0.7] * 5 + [0.0] * (nb - 19)
    low = [0.9] * 7 + [0.3] * (nb - 7)          # steps inside the first run ...
    mid = [0.5] * nb
    high = [0.1] * 16 + [0.6] * (nb - 16)       # ... and inside the second
    return [dict(occlusion=o, transmissionLow=l, transmissionMid=m, transmissionHigh=hh) for o, l, m, hh in zip(occ, low, mid, high)]


def timeline_scene(ctx, x, h, stereo):
    nb = TL_BLOCKS
    bt = M.block_times(nb, SR)
    s = source(ctx, x)
    p = panner(ctx, h, 4)
    set_params(p, POSITION)
    if stereo:
        p.SpatialBlend.Value = 0.5
    last = {}
    for b, q in enumerate(timeline_values()):
        for name, v in q.items():
            if last.get(name) != v:
                attr(p, name).SetValueAtTime(v, bt[b])
                last[name] = v
    s.Connect(p).Connect(ctx.Destination)
    return (s, p)


def timeline_input(stereo):
    frames = TL_BLOCKS * B
    return np.stack([G.voice(71, frames), G.voice(72, frames)]) if stereo else G.voice(71, frames)


_refs = {}


def timeline_reference(stereo):
    if stereo not in _refs:
        params = [dict(POSITION, **q, **({"spatialBlend": 0.5} if stereo else {})) for q in timeline_values()]
        guarded(params, TL_BLOCKS)
        ref = DM.render(timeline_input(stereo), hrir_set(), 4, params)
        ref.setflags(write=False)
        _refs[stereo] = ref
    return _refs[stereo]


def timeline_render(stereo, pieces=None, **opts):
    ctx = new_context(**opts)
    hold = timeline_scene(ctx, timeline_input(stereo), hrir_set(), stereo)
    out = render(ctx, TL_BLOCKS * B, pieces)
    ctx.Dispose()
    return out


@pytest.mark.parametrize("stereo", [False, True])
def test_timeline_of_occlusion_and_transmission(stereo):
    """a run that starts from zero state (block 4 ramps in from the identity), its ramp-out block (10), blocks that are not active
    (11 .. 13), a second run (14 ..) and its ramp-out"""
    triples = [DM.block_occlusion(q)[1] for q in timeline_values()]
    assert triples[3] == DM.EQ_IDENTITY and triples[4] != DM.EQ_IDENTITY and triples[10] == DM.EQ_IDENTITY and triples[14] != DM.EQ_IDENTITY
    assert triples[6] != triples[7] and triples[15] != triples[16]
    check(timeline_render(stereo), timeline_reference(stereo), f"timeline, stereo={stereo}")


def test_chunking_and_render_calls_are_bit_for_bit():
    whole = timeline_render(True)
    check(whole, timeline_reference(True), "chunking, whole")
    for k in (1, 3, 5):
        assert np.array_equal(timeline_render(True, max_chunk_blocks=k), whole), f"max_chunk_blocks {k}"
    assert np.array_equal(timeline_render(True, pieces=[7 * B]), whole), "two render calls that cut the first run"
    assert np.array_equal(timeline_render(True, pieces=[7 * B, 9 * B], max_chunk_blocks=3), whole), "render calls and chunks of 3"


# ---- 4. silence in the middle -----------------------------------------------------------------------------------------------------------

def test_silent_input_blocks_clear_the_state():
    """one source ends, another starts later, and transmissionLow steps during the silence: block 14 uses its own triple alone (no
    ramp from block 8's) and starts its band filters from zero"""
    nb = 20
    frames = nb * B
    h = hrir_set()
    bt = M.block_times(nb, SR)
    a, b2 = G.voice(41, 6 * B), G.voice(42, 6 * B)
    values = dict(POSITION, **WALL)
    after = dict(values, transmissionLow=0.2)
    outs = {}
    for name, (limit, pieces) in {"whole": (None, None), "chunks of 1": (1, None), "chunks of 5": (5, None),
                                  "calls": (None, [2 * B, 7 * B, 3 * B, 2 * B])}.items():
        ctx = new_context(**({"max_chunk_blocks": limit} if limit else {}))
        s1 = source(ctx, a, bt[3], bt[9])       # blocks 3 .. 8
        s2 = source(ctx, b2, bt[14])            # blocks 14 .. 19
        p = panner(ctx, h, 4)
        set_params(p, values)
        p.TransmissionLow.SetValueAtTime(0.9, 0.0)
        p.TransmissionLow.SetValueAtTime(0.2, bt[11])
        s1.Connect(p)
        s2.Connect(p)
        p.Connect(ctx.Destination)
        outs[name] = render(ctx, frames, pieces)
        ctx.Dispose()
    x = np.zeros(frames, np.float32)
    x[3 * B:9 * B] = a
    x[14 * B:20 * B] = b2
    silent = np.ones(nb, bool)
    silent[3:9] = False
    silent[14:20] = False
    params = [values] * 11 + [after] * (nb - 11)
    guarded(params, nb, silent)
    for blk in np.nonzero(silent)[0]:
        assert not outs["whole"][:, blk * B:(blk + 1) * B].any(), blk
    ref = DM.render(x, h, 4, params, silent=silent)
    triples = [DM.block_occlusion(q)[1] for q in params]
    # (without the silence rule block 14 would ramp from block 8's triple: another signal)
    ramped = DM.direct(x, triples[:9] + [triples[8]] * 5 + triples[14:])[0]
    cleared = DM.direct(x, triples, silent)[0]
    assert np.max(np.abs(ramped[14 * B:15 * B] - cleared[14 * B:15 * B])) > 1e-2
    check(outs["whole"], ref, "silence in the middle")
    for name, o in outs.items():
        assert np.array_equal(o, outs["whole"]), name


# ---- 5. a level of 70 nodes ------------------------------------------------------------------------------------------------------------

def test_mixed_level_of_70_nodes():
    """mono and stereo inputs; a third of the nodes behind a wall, a third in open air (no job), a third whose occlusion starts in the
    middle of the render: more than one wave of jobs and a partial last one"""
    nb = 12
    frames = nb * B
    bt = M.block_times(nb, SR)
    sets = [(noise_set(6 * 3, 64, 5), 6), (noise_set(4 * 1, 200, 6), 4)]
    ctx = new_context()
    shared = [HrirSet.FromArray(h, SR) for h, _ in sets]
    ref = np.zeros((2, frames))
    hold = []
    kinds = {"wall": 0, "open": 0, "late": 0}
    for v in range(70):
        which = 0 if v % 7 else 1
        h, A = sets[which]
        stereo = v % 2 == 1
        x = np.stack([G.voice(400 + v, frames), G.voice(500 + v, frames)]) if stereo else G.voice(400 + v, frames)
        ang = 2.0 * math.pi * v / 70.0
        values = dict(positionX=2.0 * math.sin(ang), positionY=0.5 * math.cos(3 * ang), positionZ=-2.0 * math.cos(ang), spatialBlend=0.6 if stereo else 1.0)
        kind = ("wall", "open", "late")[v % 3]
        occ = dict(occlusion=0.4 + 0.008 * v, transmissionLow=1.0 - 0.01 * v, transmissionMid=0.5, transmissionHigh=0.01 * v)
        s = source(ctx, x)
        p = SpatialPannerNode(ctx)
        p.HrirAzimuths = A
        p.Hrir = shared[which]
        params = values
        if kind == "wall":
            values = dict(values, **occ)
            params = values
        set_params(p, values)
        if kind == "late":
            set_params(p, {k: v_ for k, v_ in occ.items() if k != "occlusion"})
            p.Occlusion.SetValueAtTime(0.0, 0.0)
            p.Occlusion.SetValueAtTime(occ["occlusion"], bt[5])
            params = [dict(values, **dict(occ, occlusion=0.0 if b < 5 else occ["occlusion"])) for b in range(nb)]
        s.Connect(p).Connect(ctx.Destination)
        hold.append((s, p))
        kinds[kind] += 1
        guarded(params, nb)
        ref += DM.render(x, h, A, params)
    out = render(ctx, frames)
    launches = ctx.GetStats()["kernel_launches"]
    ctx.Dispose()
    print("70 nodes: kernel launches", launches)
    assert launches < 40       # one launch of the stage for the level, not one per node
    assert kinds["wall"] + kinds["late"] > 32 and all((kinds["wall"] + kinds["late"]) % k for k in (8, 16, 32))     # whatever the wave packs
    check(out, ref, "mixed level of 70")


# ---- 6. signals on occlusion and transmissionHigh (both options) -----------------------------------------------------------------

SIG_PARTS = (8, 15, 9)


def _lfo(ctx):
    o = OscillatorNode(ctx)
    o.Frequency.Value = 40.0       # a period of 9.4 blocks: occlusion is clamped to 0 for blocks at a time (runs end and start on the device)
    g = GainNode(ctx)
    g.Gain.Value = 0.8
    o.Connect(g)
    o.Start()
    return g


def signal_input(stereo):
    frames = sum(SIG_PARTS) * B
    return np.stack([G.voice(81, frames), G.voice(82, frames)]) if stereo else G.voice(81, frames)


def signal_render(stereo, chunk=None):
    nb = sum(SIG_PARTS)
    x = signal_input(stereo)
    ctx = new_context(spatial_param_signals=1, **({"max_chunk_blocks": chunk} if chunk else {}))
    s = source(ctx, x)
    p = panner(ctx, hrir_set(), 4)
    set_params(p, dict(POSITION, occlusion=0.5, transmissionLow=0.9, transmissionMid=0.5, transmissionHigh=0.1))
    if stereo:
        p.SpatialBlend.Value = 0.5
    s.Connect(p).Connect(ctx.Destination)
    out = np.zeros((2, nb * B), np.float32)
    ctx.Render(out, SIG_PARTS[0] * B, 0)
    m = _lfo(ctx)
    m.Connect(p.Occlusion)
    c = const(ctx, 0.4)
    c.Connect(p.TransmissionHigh)
    ctx.Render(out, SIG_PARTS[1] * B, SIG_PARTS[0] * B)
    m.Disconnect(p.Occlusion)
    c.Disconnect(p.TransmissionHigh)
    ctx.Render(out, SIG_PARTS[2] * B, (SIG_PARTS[0] + SIG_PARTS[1]) * B)
    ctx.Dispose()
    return out


def test_signals_on_occlusion_and_transmission():
    """8 blocks on the host's values, 15 with an oscillator on occlusion and a constant on transmissionHigh, 9 on the host's again: the
    model is fed with sample 0 of each block; the joins ramp from the triple the other side made"""
    stereo = True
    nb = sum(SIG_PARTS)
    x = signal_input(stereo)
    base = dict(POSITION, spatialBlend=0.5, occlusion=0.5, transmissionLow=0.9, transmissionMid=0.5, transmissionHigh=0.1)
    mod = mod_values(_lfo, SIG_PARTS[1])
    params = [base] * SIG_PARTS[0]
    params += [dict(base, occlusion=modulated("occlusion", 0.5, mod[b]), transmissionHigh=modulated("transmissionHigh", 0.1, 0.4)) for b in range(SIG_PARTS[1])]
    params += [base] * SIG_PARTS[2]
    occ = [q["occlusion"] for q in params[SIG_PARTS[0]:SIG_PARTS[0] + SIG_PARTS[1]]]
    print("occlusion of the signal-driven blocks:", " ".join(f"{v:.3f}" for v in occ))
    assert min(occ) == 0.0 and max(occ) > 0.9 and occ[-1] > 0.0       # clamped at both ends; the host takes over inside a run
    assert any(a == 0.0 and b > 0.0 for a, b in zip(occ, occ[1:])) and any(a > 0.0 and b == 0.0 for a, b in zip(occ, occ[1:]))
    guarded(params, nb)
    ref = DM.render(x, hrir_set(), 4, params)
    whole = signal_render(stereo)
    check(whole, ref, "signals on occlusion and transmissionHigh")
    for k in (1, 3, 5):
        assert np.array_equal(signal_render(stereo, k), whole), f"max_chunk_blocks {k}"


def test_signal_on_occlusion_needs_both_options():
    frames = 12 * B
    x = G.voice(51, frames)
    ctx = new_context()          # spatial_occlusion alone
    s = source(ctx, x)
    p = panner(ctx, hrir_set(), 4)
    set_params(p, POSITION)
    s.Connect(p).Connect(ctx.Destination)
    c = const(ctx, 0.5)
    c.Connect(p.Occlusion)
    out = np.zeros((2, frames), np.float32)
    with pytest.raises(NotSupportedException, match=r"a signal is connected to parameter 13 \(signals on the node's parameters are not on the device path\)"):
        ctx.Render(out, frames, 0)
    assert ctx.CurrentBlock == 0
    ctx.Dispose()
