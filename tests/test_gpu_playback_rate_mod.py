"""GPU parity of a k-rate playbackRate modulated by a signal (two-stage chunks: DESIGN.md "Modulated playbackRate"): the HIP path
against the CPU oracle, and the device walk (option rate_mod_walk=1) against the host replay of the read-back rates (=0)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from graphaudio_amd import (AudioBufferSourceNode, AudioStreamSourceNode, BiQuadFilterNode, ConstantSourceNode, ConvolverNode,
                            GainNode, NotSupportedException, OfflineAudioContext, OscillatorNode, PlayableAudioBuffer,
                            StereoPannerNode)
from tests import _graphs as G
from tests._oracle import OracleContext

SR = 48000
TOL_RMS = 1e-5


def render(mk, build, ch, frames, pieces=None, opts=None):
    ctx = mk(SR)
    if mk is OfflineAudioContext:
        for k, v in (opts or {}).items():
            ctx.SetOption(k, v)
    ctx.Destination.SetChannelCount(ch)
    hold = build(ctx)
    out = np.zeros((ch, frames), np.float32)
    pos = 0
    for p in (pieces or [frames]):
        k = min(p, frames - pos)
        if k <= 0:
            break
        ctx.Render(out, k, pos)
        pos += k
    if pos < frames:
        ctx.Render(out, frames - pos, pos)
    del hold
    ctx.Dispose()
    return out


def pair(build, ch, frames, pieces=None, opts=None):
    return render(OracleContext, build, ch, frames, pieces), render(OfflineAudioContext, build, ch, frames, pieces, opts)


def _lfo(ctx, freq, depth, param, start=0.0, stop=None):
    lfo = OscillatorNode(ctx)
    lfo.Frequency.Value = freq
    g = GainNode(ctx)
    g.Gain.Value = depth
    lfo.Connect(g)
    g.Connect(param)
    lfo.Start(start)
    if stop is not None:
        lfo.Stop(stop)
    return lfo, g


def _source(ctx, seed, n, sr, loop):
    s = AudioBufferSourceNode(ctx)
    s.Buffer = PlayableAudioBuffer.FromMonoArray(G.voice(seed, n), sr)
    s.Loop = loop
    return s


# ---- the cases --------------------------------------------------------------------------------------------------------------

def vibrato(ctx):
    """A looping 44.1 kHz buffer, a 5 Hz sine through a 0.05 gain into PlaybackRate."""
    s = _source(ctx, 1, 44100, 44100, True)
    hold = _lfo(ctx, 5.0, 0.05, s.PlaybackRate)
    s.Connect(ctx.Destination)
    s.Start()
    return (s,) + hold


def one_shot(ctx):
    """A one-shot whose data runs out inside a chunk under modulation, a BiQuadFilterNode behind it."""
    s = _source(ctx, 2, 128 * 60, 44100, False)
    hold = _lfo(ctx, 3.0, 0.3, s.PlaybackRate)
    bq = BiQuadFilterNode(ctx)
    bq.Frequency.Value = 2500.0
    s.Connect(bq).Connect(ctx.Destination)
    s.Start(0.01)
    return (s, bq) + hold


def clamp_and_copy(ctx):
    """A ConstantSourceNode on a timeline drives the rate below 0.001 and, at the end, above 1000 (the wrap buffer cannot feed such a
    rate: the block produces nothing and the source ends); in the other blocks it is exactly 1.0 (copy path: the buffer's rate is the
    context's)."""
    s = _source(ctx, 3, 48000, SR, True)
    cs = ConstantSourceNode(ctx)
    cs.Offset.SetValueAtTime(0.0, 0.0)
    cs.Offset.SetValueAtTime(-5.0, 0.1)
    cs.Offset.SetValueAtTime(0.0, 0.25)
    cs.Offset.SetValueAtTime(0.5, 0.45)
    cs.Offset.LinearRampToValueAtTime(2000.0, 0.7)
    cs.Connect(s.PlaybackRate)
    cs.Start()
    s.Connect(ctx.Destination)
    s.Start()
    return (s, cs)


def late_modulator(ctx):
    """The modulator starts late and stops early: in the blocks without it the rate is the intrinsic value, on a timeline of its
    own."""
    s = _source(ctx, 4, 44100, 44100, True)
    s.PlaybackRate.SetValueAtTime(1.0, 0.0)
    s.PlaybackRate.LinearRampToValueAtTime(1.5, 0.8)
    hold = _lfo(ctx, 7.0, 0.1, s.PlaybackRate, start=0.1, stop=0.5)
    s.Connect(ctx.Destination)
    s.Start()
    return (s,) + hold


def downmixed(ctx):
    """Two connections into the parameter, one of them stereo (the modulation input is down-mixed); the LFO also feeds the
    destination directly (a node of the modulator cone with a consumer in the second stage)."""
    s = _source(ctx, 5, 44100, 44100, True)
    lfo, g = _lfo(ctx, 4.0, 0.05, s.PlaybackRate)
    lfo2 = OscillatorNode(ctx)
    lfo2.Frequency.Value = 0.7
    pan = StereoPannerNode(ctx)
    pan.Pan.Value = 0.3
    g2 = GainNode(ctx)
    g2.Gain.Value = 0.02
    lfo2.Connect(pan).Connect(g2)
    g2.Connect(s.PlaybackRate)
    lfo2.Start()
    lfo.Connect(ctx.Destination)
    s.Connect(ctx.Destination)
    s.Start()
    return (s, lfo, g, lfo2, pan, g2)


def voices256(ctx):
    hold = []
    for v in range(256):
        s = _source(ctx, 100 + v, 44100 // 2, 44100, True)
        hold += [s, *_lfo(ctx, 2.0 + 0.05 * v, 0.02 + 0.0001 * v, s.PlaybackRate)]
        s.Connect(ctx.Destination)
        s.Start()
    return hold


def voices1024_conv(ctx):
    irbuf = PlayableAudioBuffer.FromChannelArrays([G.synth_ir(c, 2048) for c in range(2)], SR)
    hold = [irbuf]
    for v in range(1024):
        s = _source(ctx, 2000 + v, 128 * 90, 44100, True)
        cv = ConvolverNode(ctx)
        cv.Buffer = irbuf
        hold += [s, cv, *_lfo(ctx, 3.0 + 0.01 * v, 0.03, s.PlaybackRate)]
        s.Connect(cv).Connect(ctx.Destination)
        s.Start()
    return hold


# ---- parity with the oracle ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["default", "chunk7", "pieces"])
def test_vibrato(form):
    frames = 128 * 400
    opts = {"max_chunk_blocks": 7} if form == "chunk7" else None
    pieces = [1000, 128 * 300] if form == "pieces" else None
    ref, got = pair(vibrato, 2, frames, pieces=pieces, opts=opts)
    assert G.rms(ref) > 1e-3
    assert np.array_equal(ref, got)


def test_one_shot_runs_out_mid_chunk():
    frames = 128 * 120
    ref, got = pair(one_shot, 2, frames)
    assert G.rms(ref) > 1e-3
    assert np.abs(ref[:, -128 * 20:]).max() == 0.0   # the data ran out: silence after the END block
    assert np.array_equal(ref, got)


def test_clamp_and_copy_path():
    ref, got = pair(clamp_and_copy, 2, 128 * 300)
    assert G.rms(ref[:, :128 * 30]) > 1e-3 and G.rms(ref[:, 128 * 100:128 * 160]) > 1e-3
    assert np.array_equal(ref, got)


def test_silent_modulator_uses_intrinsic_timeline():
    ref, got = pair(late_modulator, 2, 128 * 400, opts={"max_chunk_blocks": 64})
    assert G.rms(ref) > 1e-3
    assert np.array_equal(ref, got)


def test_downmixed_modulation_and_cone_node_with_second_stage_consumer():
    ref, got = pair(downmixed, 2, 128 * 300)
    assert G.rms(ref) > 1e-3
    assert np.array_equal(ref, got)


def test_256_voices_own_lfo():
    ref, got = pair(voices256, 2, 128 * 200)
    assert G.rms(ref) > 1e-3
    assert np.array_equal(ref, got)


def test_1024_voices_into_shared_ir_convolvers():
    ref, got = pair(voices1024_conv, 2, 128 * 80)
    assert G.rms(ref) > 1e-3
    assert G.rms(ref - got) <= TOL_RMS


def test_stream_source_modulated_rate():
    def build(ctx):
        s = AudioStreamSourceNode(ctx)
        for i, (n, sr) in enumerate([(9000, 44100), (7000, 32000), (12000, 48000)]):
            s.QueueBuffer(PlayableAudioBuffer.FromMonoArray(G.voice(300 + i, n), sr))
        hold = _lfo(ctx, 6.0, 0.2, s.PlaybackRate)
        s.Connect(ctx.Destination)
        s.Play()
        return (s,) + hold
    ref, got = pair(build, 2, 128 * 250, opts={"max_chunk_blocks": 50})
    assert G.rms(ref) > 1e-3
    assert np.array_equal(ref, got)


# ---- the device walk against the host replay ----------------------------------------------------------------------------------

@pytest.mark.parametrize("case,frames", [(vibrato, 128 * 400), (one_shot, 128 * 120), (clamp_and_copy, 128 * 300),
                                         (voices256, 128 * 200), (voices1024_conv, 128 * 80)])
def test_walk_matches_host_replay(case, frames):
    walk = render(OfflineAudioContext, case, 2, frames, opts={"rate_mod_walk": 1, "max_chunk_blocks": 33})
    host = render(OfflineAudioContext, case, 2, frames, opts={"rate_mod_walk": 0, "max_chunk_blocks": 33})
    assert G.rms(walk) > 1e-3
    assert np.array_equal(walk, host)


# ---- refusals -----------------------------------------------------------------------------------------------------------------

def _refused_then_supported(make_bad):
    """The refused graph raises NotSupportedException before anything moves; with the offending connection removed, the SAME context
    renders the rest from time 0, equal to the oracle."""
    frames = 128 * 100
    ctx = OfflineAudioContext(SR)
    hold, undo = make_bad(ctx)
    out = np.zeros((2, frames), np.float32)
    with pytest.raises(NotSupportedException):
        ctx.Render(out, frames, 0)
    undo()
    ctx.Render(out, frames, 0)

    def build(octx):
        h, u = make_bad(octx)
        u()
        return h
    ref = render(OracleContext, build, 2, frames)
    del hold
    ctx.Dispose()
    assert G.rms(ref) > 1e-3
    assert np.array_equal(ref, out)


def test_nested_modulated_rates_refused():
    def make(ctx):
        inner = _source(ctx, 7, 44100, 44100, True)
        h1 = _lfo(ctx, 5.0, 0.05, inner.PlaybackRate)
        outer = _source(ctx, 8, 44100, 44100, True)
        g = GainNode(ctx)
        g.Gain.Value = 0.01
        inner.Connect(g)
        g.Connect(outer.PlaybackRate)   # the outer rate depends on a source whose own rate is modulated
        inner.Connect(ctx.Destination)
        outer.Connect(ctx.Destination)
        inner.Start()
        outer.Start()
        return (inner, outer, g) + h1, lambda: g.Disconnect(outer.PlaybackRate)
    _refused_then_supported(make)


def test_rate_feedback_refused():
    def make(ctx):
        s = _source(ctx, 9, 44100, 44100, True)
        g = GainNode(ctx)
        g.Gain.Value = 0.01
        s.Connect(g)
        g.Connect(s.PlaybackRate)   # the source's output reaches its own rate
        s.Connect(ctx.Destination)
        s.Start()
        return (s, g), lambda: g.Disconnect(s.PlaybackRate)
    _refused_then_supported(make)
