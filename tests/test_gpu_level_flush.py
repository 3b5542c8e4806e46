"""Every per-level launch queue of the chunk engine (Exec::flushLevel, ga_chunk_internal.hpp) in one small scene: each queue's table
is uploaded, launched once and cleared, level by level.

The scene puts at least one job into every queue -- down-mix, wide mix, mix, parameter modulation, looping rate-1 source, both
resample paths, general replay, stream, constant source, oscillator, constant and automated panner, spatial descriptors, spatial
panner, delay, unfolded gain (and a folded one), a two-section biquad cascade, dynamic biquad -- over more than three levels and two
control segments (sources that start inside the render).  Six blocks are rendered twice: in one piece and as pieces of 1, 2 and 3
blocks.

A ChannelMergerNode gives every class of node its own destination channels, so that each is held to its own condition:
  0, 1  the nodes that are bit for bit against the oracle                                       np.array_equal, plain oracle
  2, 3  the kernels that evaluate moving parameters (dynamic biquad, automated panner)          np.array_equal, double-trig oracle
        (the device evaluates cos / sin as (float)cos((double)x): tests/test_gpu_param_edges.py)
  4     the oscillator: the bound of tests/test_gpu_nodes2.py::test_oscillator_types_bit_exact  max-abs <= 1.2e-7 (one float ulp)
  6, 7  the spatial panners (static and signal-driven) against the float64 model                tests/test_gpu_spatial.py::check
A queue that is launched twice or not cleared rewrites the same values, which no output shows; the launch counters do: they count one
per recorded launch.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from graphaudio_amd import (AudioBufferSourceNode, AudioStreamSourceNode, BiQuadFilterNode, ChannelCountMode, ChannelMergerNode,
                            ChannelSplitterNode, ConstantSourceNode, DelayNode, GainNode, OfflineAudioContext, OscillatorNode,
                            PlayableAudioBuffer, StereoPannerNode)
from tests import _graphs as G
from tests import _spatial_model as M
from tests._oracle import DtrigOracleContext, OracleContext
from tests.test_gpu_spatial import check, noise_set, panner, set_params, source
from tests.test_gpu_spatial_signals import modulated

SR = 48000
B = 128
NB = 6
FRAMES = NB * B
CHANNELS = 8
PIECES = {"one piece": [6 * B], "pieces of 1, 2 and 3 blocks": [1 * B, 2 * B, 3 * B]}

# GetStats() of the PARENT commit's library (the one before Exec::flush existed) for this scene, measured once on an MI355X by loading
# that build through graphaudio_amd._capi.use_library: the refactor records the same launches.
PARENT_KERNEL_LAUNCHES = {"one piece": 86, "pieces of 1, 2 and 3 blocks": 95}
PARENT_STAGE_LAUNCHES = {"one piece": [70, 16] + [0] * 14, "pieces of 1, 2 and 3 blocks": [79, 16] + [0] * 14}

SPATIAL_HRIR, SPATIAL_A = noise_set(12, 33, 3), 4
SPATIAL_STATIC = dict(positionX=-2.0, positionY=0.5, positionZ=1.0)
SPATIAL_DRIVEN = dict(positionX=1.0, positionY=-0.5, positionZ=0.8)    # positionX + a constant signal of 0.5
SPATIAL_X = [G.voice(61, FRAMES), G.voice(62, FRAMES)]


def mono(ctx, seed, n, sr=SR):
    s = AudioBufferSourceNode(ctx)
    s.Buffer = PlayableAudioBuffer.FromMonoArray(G.voice(seed, n), sr)
    return s


def gain(ctx, value):
    g = GainNode(ctx)
    g.Gain.Value = value
    return g


def scene(ctx, spatial):
    """-> everything that has to stay alive.  `spatial`: with the spatial panners (the oracles do not have the node)"""
    ctx.Destination.SetChannelCount(CHANNELS)
    merger = ChannelMergerNode(ctx, CHANNELS)
    merger.Connect(ctx.Destination)
    hold = [merger]

    def bus(first_channel):
        b, sp = GainNode(ctx), ChannelSplitterNode(ctx, 2)     # a unity gain hands its mixed input on
        b.Inputs[0].SetChannelCount(2)
        b.Inputs[0].SetChannelCountMode(ChannelCountMode.Explicit)
        b.Connect(sp)
        sp.Connect(merger, 0, first_channel)
        sp.Connect(merger, 1, first_channel + 1)
        hold.extend([b, sp])
        return b

    # ---- channels 0, 1: bit for bit against the oracle ----
    exact = bus(0)
    cs = ConstantSourceNode(ctx)                               # constant source
    cs.Offset.Value = 0.1
    cs.Connect(exact)
    cs.Start(0.0)
    loop1 = mono(ctx, 1, 300)                                  # looping source at rate 1, behind a folded gain (one consumer)
    loop1.Loop = True
    loop1.Connect(gain(ctx, 0.7)).Connect(exact)
    loop1.Start(0.0)
    rs = mono(ctx, 2, 3000, 44100)                             # 44.1 kHz in a 48 kHz context, from inside block 1: a second segment
    unfolded = gain(ctx, 0.6)                                  # two consumers: a pass of its own
    delay = DelayNode(ctx, 0.02)                               # level 3: source -> gain -> delay -> bus
    delay.DelayTime.Value = 0.003
    rs.Connect(unfolded)
    unfolded.Connect(exact)
    unfolded.Connect(delay).Connect(exact)
    rs.Start(0.004)
    short = mono(ctx, 8, 200, 44100)                           # ... and one that runs out inside block 1: the partial block's path
    short.Connect(exact)
    short.Start(0.0)
    replay = mono(ctx, 3, 700, 44100)                          # looping AND resampled: the general replay; a constant panner
    replay.Loop = True
    replay.LoopStart = 300 / 44100
    pan = StereoPannerNode(ctx)
    pan.Pan.Value = 0.3
    replay.Connect(pan).Connect(exact)
    replay.Start(0.0)
    stream = AudioStreamSourceNode(ctx)                        # stream source in front of a two-section cascade
    for i, (n, sr) in enumerate([(500, 44100), (900, SR)]):
        stream.QueueBuffer(PlayableAudioBuffer.FromMonoArray(G.voice(10 + i, n), sr))
    bq1, bq2 = BiQuadFilterNode(ctx), BiQuadFilterNode(ctx)
    bq1.Frequency.Value = 1200.0
    bq2.Frequency.Value = 3000.0
    bq2.Q.Value = 2.0
    stream.Connect(bq1).Connect(bq2).Connect(exact)
    stream.Play()
    st = AudioBufferSourceNode(ctx)                            # a stereo producer into an explicit mono input: the down-mix
    st.Buffer = PlayableAudioBuffer.FromStereoArrays(G.voice(4, FRAMES + 256), G.voice(5, FRAMES + 256), SR)
    down = gain(ctx, 0.5)
    down.Inputs[0].SetChannelCount(1)
    down.Inputs[0].SetChannelCountMode(ChannelCountMode.Explicit)
    st.Connect(down).Connect(exact)
    st.Start(0.002)
    wide = GainNode(ctx)                                       # a bus of 256 terms: the wide mix
    for v in range(256):
        c = ConstantSourceNode(ctx)
        c.Offset.Value = (v % 17 - 8) / 1024.0
        c.Connect(wide)
        c.Start(0.0)
        hold.append(c)
    wide.Connect(exact)
    hold.extend([cs, loop1, rs, short, unfolded, delay, replay, pan, stream, bq1, bq2, st, down, wide])

    # ---- channels 2, 3: moving parameters, bit for bit against the double-trig oracle ----
    moving = bus(2)
    lfo = AudioBufferSourceNode(ctx)                           # a signal on a biquad's frequency: parameter modulation + dynamic biquad
    lfo.Buffer = PlayableAudioBuffer.FromMonoArray((0.4 * np.sin(2 * np.pi * np.arange(480) / 240.0)).astype(np.float32), SR)
    lfo.Loop = True
    depth = gain(ctx, 2000.0)
    wah = BiQuadFilterNode(ctx)
    wah.Frequency.Value = 2500.0
    lfo.Connect(depth)
    depth.Connect(wah.Frequency)
    v1 = mono(ctx, 6, FRAMES + 256)
    v1.Connect(wah).Connect(moving)
    sweep = StereoPannerNode(ctx)                              # a pan on a timeline: the automated panner
    sweep.Pan.SetValueAtTime(-0.5, 0.0)
    sweep.Pan.LinearRampToValueAtTime(0.5, 0.01)
    v2 = mono(ctx, 7, FRAMES + 256)
    v2.Connect(sweep).Connect(moving)
    lfo.Start(0.0)
    v1.Start(0.0)
    v2.Start(0.0)
    hold.extend([lfo, depth, wah, v1, sweep, v2])

    # ---- channel 4: the oscillator ----
    osc = OscillatorNode(ctx)
    osc.Frequency.Value = 997.0
    osc.Connect(merger, 0, 4)
    osc.Start(0.0)
    hold.append(osc)

    # ---- channels 6, 7: spatial panners, one static and one with a signal on positionX ----
    if spatial:
        room = bus(6)
        for x, values in zip(SPATIAL_X, (SPATIAL_STATIC, SPATIAL_DRIVEN)):
            s, p = source(ctx, x), panner(ctx, SPATIAL_HRIR, SPATIAL_A)
            set_params(p, values)
            s.Connect(p).Connect(room)
            hold.extend([s, p])
        c = ConstantSourceNode(ctx)
        c.Offset.Value = 0.5
        c.Connect(p.PositionX)                                 # (the second panner)
        c.Start()
        hold.append(c)
    return hold


def render(make, pieces, spatial=False):
    ctx = make(SR)
    if spatial:
        ctx.SetOption("spatial_param_signals", 1)
    hold = scene(ctx, spatial)
    out = np.zeros((CHANNELS, FRAMES), np.float32)
    pos = 0
    for k in pieces:
        ctx.Render(out, k, pos)
        pos += k
    assert pos == FRAMES
    stats = ctx.GetStats() if spatial else None
    del hold
    ctx.Dispose()
    return out, stats


@pytest.fixture(scope="module")
def references():
    plain, _ = render(OracleContext, [FRAMES])
    dtrig, _ = render(DtrigOracleContext, [FRAMES])
    driven = dict(SPATIAL_DRIVEN, positionX=modulated("positionX", SPATIAL_DRIVEN["positionX"], 0.5))
    room = M.render(SPATIAL_X[0], SPATIAL_HRIR, SPATIAL_A, SPATIAL_STATIC) + M.render(SPATIAL_X[1], SPATIAL_HRIR, SPATIAL_A, driven)
    for r in (plain, dtrig, room):
        r.setflags(write=False)
    return plain, dtrig, room


@pytest.mark.parametrize("how", list(PIECES))
def test_every_level_queue_is_launched_once(how, references):
    plain, dtrig, room = references
    got, stats = render(OfflineAudioContext, PIECES[how], spatial=True)
    print(f"{how}: kernel_launches {stats['kernel_launches']} stage_launches {list(stats['stage_launches'])}")
    for lo in (0, 2, 4, 6):
        ref = room if lo == 6 else (dtrig if lo == 2 else plain)[lo:lo + 2]
        d = np.abs(got[lo:lo + 2].astype(np.float64) - ref)
        print(f"{how}: channels {lo}, {lo + 1}: rms {G.rms(got[lo:lo + 2]):.3e}  max-abs difference {d.max():.3e}  differing samples {int(np.count_nonzero(d))}")
    assert min(G.rms(plain[ch]) for ch in (0, 1, 4)) > 1e-2 and min(G.rms(dtrig[ch]) for ch in (2, 3)) > 1e-2
    assert not got[5].any() and not plain[5].any()
    assert np.array_equal(got[0:2], plain[0:2])
    assert np.array_equal(got[2:4], dtrig[2:4])
    assert np.abs(got[4] - plain[4]).max() <= 1.2e-7     # sin(double) differs in the double's last bit: at most one float ulp below 1
    check(got[6:8], room, "spatial panners, " + how)
    assert stats["kernel_launches"] == PARENT_KERNEL_LAUNCHES[how]
    assert list(stats["stage_launches"]) == PARENT_STAGE_LAUNCHES[how]
