"""DynamicsCompressorNode in scenes only the CPU oracle can check: the compressor's output feeds other nodes
and parameters, so the destination no longer shows its input and the float64 model cannot be fed.  The oracle's node is pinned to that
model without a GPU (tests/test_oracle_compressor.py); here the device is held to the oracle.

Where the compressor's input is bit-identical on both sides (a buffer source at the context's rate), its output -- shown on a channel
of its own through a ChannelMergerNode -- is within M.TOL = 2^-22 |m| of the oracle's m, sample by sample, exact zeros included.
Downstream of it the fuzzers' contract holds: rms error <= 1e-5 max(1, rms) and <= 2e-5 rms.  The device renders in uneven pieces."""
import numpy as np
import pytest

from graphaudio_amd import (AudioBufferSourceNode, BiQuadFilterNode, ChannelMergerNode, ConvolverNode, DynamicsCompressorNode, FilterType,
                            GainNode, OfflineAudioContext, PlayableAudioBuffer)
from tests import _compressor_model as M
from tests import _graphs as G
from tests._oracle import OracleContext

pytestmark = pytest.mark.gpu
FS = 48000
BLOCKS = 12
PIECES = [200, 1000, 336]   # a partial block, a long piece, the rest


def _compressor(ctx, **values):
    cm = DynamicsCompressorNode(ctx)
    for name, v in values.items():
        getattr(cm, name[0].upper() + name[1:]).Value = v
    return cm


def _source(ctx, seed, channels=1, levels=(-12.0, -40.0, 0.0), loop=False, frames=BLOCKS * 128 + 512):
    x = M.bursts(seed, frames, channels=channels, levels_db=levels, burst=300, gap=150)
    s = AudioBufferSourceNode(ctx)
    s.Buffer = PlayableAudioBuffer.FromChannelArrays([np.ascontiguousarray(r) for r in x], FS)
    s.Loop = loop
    s.Start()
    return s


def _pair(build, options=(), pieces=PIECES, between=None):
    """build(ctx) on the oracle (one Render call) and on the device (one per piece); `between(handles, piece index)` edits both"""
    outs = []
    for device in (False, True):
        ctx = OfflineAudioContext(FS, device=0) if device else OracleContext(FS)
        if device:
            ctx.SetOption("max_chunk_blocks", 11)
            for k, v in options:
                ctx.SetOption(k, v)
        handles = build(ctx)
        out = np.zeros((2, sum(pieces)), dtype=np.float32)
        at = 0
        for i, n in enumerate(pieces if device or between else [sum(pieces)]):
            ctx.Render(out, n, at)
            at += n
            if between:
                between(handles, i)
        outs.append(out)
    return outs


def _node_output_holds(got, ref, name):
    print(f"{name}: compressor output, worst |y - m| / |m| = {M.worst(got, ref):.3e} (bound {M.TOL:.3e})")
    assert np.any(ref != 0)
    assert M.within(got, ref)


def _contract_holds(got, ref, name):
    err, rms = G.rms(ref - got), G.rms(ref)
    print(f"{name}: rms {rms:.3e}, rms error {err:.3e}")
    scale = max(rms, 1e-3)
    assert rms > 1e-3
    assert err <= 1e-5 * max(1.0, scale) and err <= 2e-5 * scale, (name, err, scale)


def _merged(ctx, first, second):
    mg = ChannelMergerNode(ctx, 2)
    first.Connect(mg, 0, 0)
    second.Connect(mg, 0, 1)
    mg.Connect(ctx.Destination)


def test_compressor_into_a_biquad():
    def build(ctx):
        cm = _compressor(ctx, threshold=-30.0, ratio=6.0, release=0.03)
        bq = BiQuadFilterNode(ctx)
        bq.Type = FilterType.Peaking
        bq.Frequency.Value = 900.0
        bq.Q.Value = 1.5
        bq.Gain.Value = 6.0
        _source(ctx, 101).Connect(cm).Connect(bq)
        _merged(ctx, cm, bq)
    ref, got = _pair(build)
    _node_output_holds(got[0], ref[0], "-> biquad")
    _contract_holds(got[1], ref[1], "-> biquad, behind the biquad")
    assert not np.array_equal(ref[0], ref[1])


@pytest.mark.parametrize("coarse", [0, 1])
def test_compressors_in_front_of_a_shared_ir_convolver_group(coarse):
    ir = [G.synth_ir(c, 256) for c in range(2)]

    def build(ctx):
        buf = PlayableAudioBuffer.FromChannelArrays(ir, FS)
        for v in range(6):
            cm = _compressor(ctx, threshold=-20.0 - 4.0 * v, ratio=2.0 + v, attack=0.0 if v == 3 else 0.003, makeupGain=float(v - 2))
            cv = ConvolverNode(ctx)
            cv.Buffer = buf
            _source(ctx, 110 + v, channels=1 + v % 2).Connect(cm).Connect(cv).Connect(ctx.Destination)
    ref, got = _pair(build, options=(("coarse_min_blocks", 1 if coarse else 1 << 30),))
    _contract_holds(got, ref, f"-> shared-IR group (coarse {coarse})")


def test_compressor_output_into_another_sources_playback_rate():
    """a two-stage chunk with the compressor in the first stage: looping noise -> compressor -> depth gain -> PlaybackRate"""
    def build(ctx):
        cm = _compressor(ctx, threshold=-35.0, ratio=10.0, attack=0.001, release=0.01, makeupGain=3.0)
        dg = GainNode(ctx)
        dg.Gain.Value = 0.25
        _source(ctx, 121, loop=True, frames=700, levels=(-6.0, -30.0)).Connect(cm).Connect(dg)
        voice = _source(ctx, 122, channels=2, frames=4 * BLOCKS * 128, levels=(-10.0,))
        dg.Connect(voice.PlaybackRate)
        voice.Connect(ctx.Destination)
    ref, got = _pair(build)
    _contract_holds(got, ref, "-> PlaybackRate")

    def plain(ctx):   # (the modulation is audible: the same voice at its own rate is another signal)
        _source(ctx, 122, channels=2, frames=4 * BLOCKS * 128, levels=(-10.0,)).Connect(ctx.Destination)
    assert G.rms(_pair(plain)[0] - ref) > 1e-2


def test_compressor_output_into_a_gain_nodes_gain():
    def build(ctx):
        cm = _compressor(ctx, threshold=-40.0, knee=0.0, ratio=20.0, release=0.005)
        dg = GainNode(ctx)
        dg.Gain.Value = 0.8
        g = GainNode(ctx)
        g.Gain.Value = 0.5
        _source(ctx, 131, levels=(-3.0, -50.0, -20.0)).Connect(cm).Connect(dg)
        dg.Connect(g.Gain)
        _source(ctx, 132, levels=(-8.0,)).Connect(g)
        _merged(ctx, cm, g)
    ref, got = _pair(build)
    _node_output_holds(got[0], ref[0], "-> gain.Gain")
    _contract_holds(got[1], ref[1], "-> gain.Gain, behind the gain")


def test_loop_without_a_delay_through_a_compressor():
    """source -> gain -> compressor -> gain 0.3 -> back into the first gain: chunks of one block.  Channel 1 shows the compressor's
    input; where it is bit-identical to the oracle's, the output is held to M.TOL, otherwise to the contract."""
    def build(ctx):
        gi = GainNode(ctx)
        gi.Gain.Value = 0.6
        cm = _compressor(ctx, threshold=-35.0, ratio=5.0, attack=0.0005, release=0.02, makeupGain=-2.0)
        fb = GainNode(ctx)
        fb.Gain.Value = 0.3
        _source(ctx, 141, levels=(0.0, -12.0, -30.0)).Connect(gi).Connect(cm).Connect(fb).Connect(gi)
        _merged(ctx, cm, gi)
    ref, got = _pair(build)
    _contract_holds(got, ref, "loop")
    if np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32)):
        _node_output_holds(got[0], ref[0], "loop")
    else:
        print("loop: the compressor's input differs in its last bits; held to the contract alone")


@pytest.mark.parametrize("what", ["compressor", "source"])
def test_unplugged_for_three_blocks_between_render_calls(what):
    """the compressor taken out: it is not pulled, yL must stand still (and its source resumes where it was); its source taken out:
    the compressor is pulled with a silent input, yL must decay for three blocks"""
    def build(ctx):
        cm = _compressor(ctx, threshold=-30.0, ratio=8.0, release=0.2)
        s = _source(ctx, 151, channels=2, levels=(-6.0, -25.0))
        s.Connect(cm).Connect(ctx.Destination)
        return ctx, s, cm

    def between(handles, i):
        ctx, s, cm = handles
        n, to = (cm, ctx.Destination) if what == "compressor" else (s, cm)
        if i == 0:
            n.Disconnect()
        elif i == 1:
            n.Connect(to)
    ref, got = _pair(build, pieces=[4 * 128 + 40, 3 * 128, 5 * 128 - 40], between=between)
    gap = slice(5 * 128, 7 * 128)   # (the blocks that lie entirely between the two edits)
    assert np.all(ref[:, gap] == 0) and np.any(ref[:, :4 * 128] != 0) and np.any(ref[:, 8 * 128:] != 0)
    _node_output_holds(got, ref, f"{what} unplugged")


def test_two_compressors_in_series():
    def build(ctx):
        first = _compressor(ctx, threshold=-30.0, ratio=3.0, release=0.05, makeupGain=8.0)
        second = _compressor(ctx, threshold=-12.0, knee=0.0, ratio=20.0, attack=0.0, release=0.01)   # a limiter behind it
        _source(ctx, 161, levels=(-3.0, -35.0, -15.0)).Connect(first).Connect(second)
        _merged(ctx, first, second)
    ref, got = _pair(build)
    _node_output_holds(got[0], ref[0], "series, first")
    if np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)):
        _node_output_holds(got[1], ref[1], "series, second")
    _contract_holds(got[1], ref[1], "series, second")
