"""DynamicsCompressorNode through the Python host, held to the float64 model of tests/_compressor_model.py:
every sample within 2^-22 |m| of the model m (two float ulps: tests/test_gpu_compressor_kernel.py says where they come from), exact
zeros where the model is exactly 0.

The model is fed the node's input as the existing path renders it: the same graph with the compressor replaced by a unity GainNode
whose input is configured like the compressor's (2 channels, clamped-max, speakers), so the mix in front of it -- channel count of
every block included -- is the compressor's.  The destination shows a mono block on two equal channels, and the link of two equal
channels is the link of one, so the model always runs on the destination's two channels."""
import numpy as np
import pytest

from graphaudio_amd import (AudioBufferSourceNode, ChannelCountMode, ChannelInterpretation, ChannelMergerNode, ConvolverNode, DelayNode,
                            DynamicsCompressorNode, GainNode, NotSupportedException, OfflineAudioContext, OscillatorNode,
                            PlayableAudioBuffer)
from tests import _compressor_model as M
from tests import _graphs as G

pytestmark = pytest.mark.gpu
FS = 48000


def _stand_in(ctx):
    g = GainNode(ctx)
    g.Inputs[0].SetChannelCount(2)
    g.Inputs[0].SetChannelCountMode(ChannelCountMode.ClampedMax)
    g.Inputs[0].SetChannelInterpretation(ChannelInterpretation.Speakers)
    return g


def _compressor(ctx, **values):
    cm = DynamicsCompressorNode(ctx)
    for name, v in values.items():
        getattr(cm, name[0].upper() + name[1:]).Value = v
    return cm


def _source(ctx, seed, frames, channels=1, levels=(-12.0, -40.0, 0.0), start=0.0):
    x = M.bursts(seed, frames + 256, channels=channels, levels_db=levels, burst=300, gap=150)
    s = AudioBufferSourceNode(ctx)
    s.Buffer = PlayableAudioBuffer.FromChannelArrays([np.ascontiguousarray(r) for r in x], FS)
    s.Start(start)
    return s


def _render(build, node, frames, calls=None, options=()):
    """the destination's two channels of build(ctx, node(ctx)) -- in one Render call or one per entry of `calls`"""
    ctx = OfflineAudioContext(FS, device=0)
    for k, v in options:
        ctx.SetOption(k, v)
    build(ctx, node(ctx))
    out = np.zeros((2, frames), dtype=np.float32)
    at = 0
    for n in calls or [frames]:
        ctx.Render(out, n, at)
        at += n
    assert at == frames
    return out


def _check(build, frames, values=None, pars=None, options=(), name=""):
    """render with the stand-in, feed the model, render with the compressor, compare; returns the compressor's render"""
    values = values or {}
    x = _render(build, _stand_in, frames, options=options)
    y = _render(build, lambda ctx: _compressor(ctx, **values), frames, options=options)
    m = M.Compressor(FS).process(x, pars if pars is not None else M.block_params(FS, **values))
    print(f"{name}: input rms {G.rms(x):.3e}, worst |y - m| / |m| = {M.worst(y, m):.3e} (bound {M.TOL:.3e})")
    assert np.any(m != 0) and not np.array_equal(m, x)   # (the compressor did something)
    assert M.within(y, m)
    return y


def _chain(channels, seed=11):
    def build(ctx, node):
        _source(ctx, seed, 8 * 128, channels=channels).Connect(node).Connect(ctx.Destination)
    return build


@pytest.mark.parametrize("channels", [1, 2])
def test_source_compressor_destination(channels):
    _check(_chain(channels), 8 * 128, name=f"chain {channels} ch")
    _check(_chain(channels, seed=12), 8 * 128, values=dict(threshold=-35.0, knee=0.0, ratio=20.0, attack=0.0, release=0.02, makeupGain=9.0),
           name=f"limiter {channels} ch")


def test_input_goes_from_one_to_two_channels_in_mid_render():
    def build(ctx, node):
        _source(ctx, 21, 8 * 128, channels=1).Connect(node)
        _source(ctx, 22, 8 * 128, channels=2, levels=(0.0, -12.0, -40.0), start=3.5 * 128 / FS).Connect(node)   # (starts inside block 3)
        node.Connect(ctx.Destination)
    y = _check(build, 8 * 128, values=dict(threshold=-30.0, ratio=6.0), name="1 -> 2 channels")
    assert np.array_equal(y[0, :3 * 128], y[1, :3 * 128]) and not np.array_equal(y[0, 5 * 128:], y[1, 5 * 128:])


def _linear(v0, t0, v1, t1, t):
    """AudioParam's linear ramp as the library evaluates it (float end points, double interpolation, rounded to float)"""
    u = min(max((t - t0) / (t1 - t0), 0.0), 1.0)
    d = np.float32(v1) - np.float32(v0)
    return float(np.float32(float(np.float32(v0)) + float(d) * u))


def test_threshold_on_a_timeline():
    frames, t1 = 8 * 128, 5.5 * 128 / FS

    def node(ctx):
        cm = _compressor(ctx, ratio=8.0, knee=6.0)
        cm.Threshold.SetValueAtTime(-10.0, 0.0)
        cm.Threshold.LinearRampToValueAtTime(-45.0, t1)
        return cm
    x = _render(_chain(2, seed=31), _stand_in, frames)
    y = _render(_chain(2, seed=31), node, frames)
    pars, t = [], 0.0
    for _ in range(8):   # the value at the block's start, on the accumulated block clock
        pars.append(M.block_params(FS, ratio=8.0, knee=6.0, threshold=_linear(-10.0, 0.0, -45.0, t1, t) if t < t1 else -45.0))
        t += 128 / FS
    assert len({p[0] for p in pars}) == 7
    m = M.Compressor(FS).process(x, pars)
    print(f"timeline: worst |y - m| / |m| = {M.worst(y, m):.3e} (bound {M.TOL:.3e})")
    assert M.within(y, m)


def test_two_render_calls_with_a_partial_block_equal_one():
    node = lambda ctx: _compressor(ctx, threshold=-30.0, release=0.01)
    one = _render(_chain(2, seed=41), node, 512)
    two = _render(_chain(2, seed=41), node, 512, calls=[200, 312])
    assert np.any(one != 0)
    assert np.array_equal(one.view(np.uint32), two.view(np.uint32))


@pytest.mark.parametrize("cycle_delay_split", [1, 0])
def test_compressor_inside_a_feedback_loop(cycle_delay_split):
    """source -> [gain 0.3] -> delay of 256 frames -> compressor -> back into the gain.  Channel 0 of the destination is the
    compressor's output, channel 1 the delay's: the loop's own rendered input, which drives the model block by block.  With
    cycle_delay_split = 0 the loop renders in chunks of one block, with 1 it is cut at the delay."""
    frames = 8 * 128
    ctx = OfflineAudioContext(FS, device=0)
    ctx.SetOption("cycle_delay_split", cycle_delay_split)
    src = _source(ctx, 51, frames, levels=(0.0, -12.0, 0.0))
    g = GainNode(ctx)
    g.Gain.Value = 0.3
    dl = DelayNode(ctx, 0.1)
    dl.DelayTime.Value = 256.5 / FS   # (int)(delayTime * sampleRate) = 256
    cm = _compressor(ctx, threshold=-40.0, ratio=4.0, attack=0.001, release=0.02, makeupGain=6.0)
    mg = ChannelMergerNode(ctx, 2)
    src.Connect(g)
    g.Connect(dl).Connect(cm).Connect(g)
    cm.Connect(mg, 0, 0)
    dl.Connect(mg, 0, 1)
    mg.Connect(ctx.Destination)
    out = np.zeros((2, frames), dtype=np.float32)
    ctx.Render(out, frames)
    y, x = out[0], out[1]
    assert np.all(x[:256] == 0) and np.any(x[256:] != 0)
    model = M.Compressor(FS)
    pars = M.block_params(FS, threshold=-40.0, ratio=4.0, attack=0.001, release=0.02, makeupGain=6.0)
    m = np.concatenate([model.process(x[None, b * 128:(b + 1) * 128], pars)[0] for b in range(8)])
    print(f"loop (cycle_delay_split {cycle_delay_split}): worst |y - m| / |m| = {M.worst(y, m):.3e} (bound {M.TOL:.3e})")
    assert np.any(m != 0)
    assert M.within(y, m)


def test_behind_a_modulated_playback_rate():
    """a two-stage chunk: the source's playbackRate is modulated by a signal, the compressor is planned in the second stage"""
    def build(ctx, node):
        s = _source(ctx, 61, 2 * 8 * 128, channels=2)
        lfo = OscillatorNode(ctx)
        lfo.Frequency.Value = 40.0
        lg = GainNode(ctx)
        lg.Gain.Value = 0.2
        lfo.Connect(lg)
        lg.Connect(s.PlaybackRate)
        lfo.Start()
        s.Connect(node).Connect(ctx.Destination)
    _check(build, 8 * 128, values=dict(threshold=-30.0), name="modulated rate")


def test_bus_compressor_behind_a_shared_ir_group_leaves_the_bus_alone():
    """16 sources -> 16 convolvers on one 256-tap impulse response -> one bus.  With ratio 1 and makeupGain 0 the gain is exactly 1,
    so the destination must be bit-identical to the same graph with a unity GainNode (gain_pass_through = 0: a node with a kernel
    of its own) in the compressor's place: the node disturbs neither the convolvers' grouping nor their formulation."""
    frames = 8 * 128
    ir = PlayableAudioBuffer.FromChannelArrays([G.synth_ir(c, 256) for c in range(2)], FS)

    def build(ctx, node):
        for v in range(16):
            s = AudioBufferSourceNode(ctx)
            s.Buffer = PlayableAudioBuffer.FromMonoArray(G.voice(v, frames + 256), FS)
            cv = ConvolverNode(ctx)
            cv.Buffer = ir
            s.Connect(cv).Connect(node)
            s.Start()
        node.Connect(ctx.Destination)
    opts = (("gain_pass_through", 0),)
    want = _render(build, _stand_in, frames, options=opts)
    got = _render(build, lambda ctx: _compressor(ctx, ratio=1.0, makeupGain=0.0), frames, options=opts)
    assert G.rms(want) > 1e-3
    assert np.array_equal(want.view(np.uint32), got.view(np.uint32))
    # ... and a bus compressor that does compress follows the model there
    _check(build, frames, values=dict(threshold=-30.0, ratio=4.0), options=opts, name="bus")


def test_long_chunk_of_260_blocks():
    frames = 260 * 128

    def build(ctx, node):
        _source(ctx, 71, frames, channels=2).Connect(node).Connect(ctx.Destination)
    values = dict(threshold=-28.0, knee=12.0, ratio=5.0, release=0.08)
    y = _check(build, frames, values=values, name="260 blocks")
    halves = _render(build, lambda ctx: _compressor(ctx, **values), frames, calls=[130 * 128, 130 * 128])
    assert np.array_equal(y.view(np.uint32), halves.view(np.uint32))


def test_a_signal_on_a_parameter_is_refused_and_names_it():
    ctx = OfflineAudioContext(FS, device=0)
    cm = DynamicsCompressorNode(ctx)
    osc = OscillatorNode(ctx)
    for p in (cm.Ratio, cm.Threshold, cm.MakeupGain):
        with pytest.raises(NotSupportedException) as e:
            osc.Connect(p)
        assert p.Name in str(e.value)
    _source(ctx, 81, 256).Connect(cm).Connect(ctx.Destination)   # the context is as it was: it renders
    out = np.zeros((2, 256), dtype=np.float32)
    ctx.Render(out, 256)
    assert np.any(out != 0)


def test_out_of_range_values_are_clamped_not_refused():
    ctx = OfflineAudioContext(FS, device=0)
    cm = DynamicsCompressorNode(ctx)
    for p, v, want in ((cm.Threshold, 5.0, 0.0), (cm.Threshold, -500.0, -100.0), (cm.Knee, 41.0, 40.0), (cm.Ratio, 0.5, 1.0), (cm.Ratio, 50.0, 20.0),
                       (cm.Attack, -1.0, 0.0), (cm.Release, 2.0, 1.0), (cm.MakeupGain, 100.0, 40.0)):
        p.Value = v
        assert p.Value == want
    values = dict(threshold=-500.0, knee=41.0, ratio=50.0, attack=-1.0, release=2.0, makeupGain=-100.0)
    _check(_chain(2, seed=91), 8 * 128, values=values, name="clamped")   # (the model clamps to the same ranges)
