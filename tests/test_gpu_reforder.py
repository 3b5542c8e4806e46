"""Formulation R: the convolver's partition sum in the reference's own order and arithmetic (refmac_kernel: separately rounded
float32 multiplies / subtracts / adds, partitions ascending, PartitionedConvolver.cs:154-223) between double-precision 256-point
transforms (FftFlat's precision).  Unlike formulations A-D, which associate the sum differently (~4-8e-7 relative), this route has
to reproduce the oracle's float32 output BIT FOR BIT -- up to the ~1e-9 chance per value that two correct double-precision
transforms round to different floats.  The planner takes it where a convolver's output reaches arithmetic that amplifies or
quantises last-bit differences (Context::refOrderSensitivity); option conv_reference_order = 2 forces it everywhere."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from graphaudio_amd import (AudioBufferSourceNode, BiQuadFilterNode, ConvolverNode, DelayNode, FilterType, GainNode,
                            OfflineAudioContext, PlayableAudioBuffer, StereoPannerNode)
from tests import _graphs as G
from tests._oracle import OracleContext
from tests._report import note

SR = 48000


def flips(ref, got):
    """(values that differ, largest difference relative to the larger value)"""
    d = ref != got
    n = int(d.sum())
    if n == 0:
        return 0, 0.0
    rel = np.abs(ref[d].astype(np.float64) - got[d]) / np.maximum(np.abs(ref[d]), 1e-30)
    return n, float(rel.max())


def render_pair(builder, frames, pieces=None, **opts):
    o = OracleContext(SR)
    ch = builder(o)
    ref = G.render(o, ch, frames)
    h = OfflineAudioContext(SR)
    for k, v in opts.items():
        h.SetOption(k, v)
    builder(h)
    got = np.zeros_like(ref)
    pos = 0
    for n in (pieces or [frames]):
        n = min(n, frames - pos)
        if n > 0:
            h.Render(got, n, pos)
            pos += n
    if pos < frames:
        h.Render(got, frames - pos, pos)
    st = h.GetStats()
    h.Dispose()
    o.Dispose()
    return ref, got, st


# What "bit for bit" means here.  The oracle's double-precision transform (a radix-2 FFT) and the device's (radix-2 butterflies
# across lanes, fma in the twiddle products) are both correct to ~1e-16 of the block's norm but not the same operation sequence --
# and neither is Ooura's fftsg, which the reference vendors: where an exact spectrum value lies within that distance of a float32
# rounding boundary the two casts (PartitionedConvolver.cs:117-118,148-149) land on neighbouring floats.  Such a flip is rare per
# value (1e-8 .. 1e-6, the smaller the value against the block's norm the likelier) but one flipped spectrum value enters P x 128
# output samples, so at P = 512 a few output samples per 100,000 end up one float32 step away.  The partition sum itself adds
# nothing: with short impulse responses (few products per flip) whole renders compare equal (test_tap_counts_bit_equal).
def test_config3_sixteen_voices_65536_taps_bit_equal():
    """VERDICT r3 item 2's bar: config 3 at 16 voices x 65,536 taps (P = 512, all partitions live), every value compared."""
    frames = 128 * 600
    ref, got, st = render_pair(lambda c: G.config3_convolver(c, voices=16, taps=65536, frames=frames), frames, conv_reference_order=2)
    assert st["ref_order_rows"] == 32 and st["stage_launches"][5] == 0   # every channel-instance on R, no coarse-partition launch
    n, worst = flips(ref, got)
    err = G.rms(ref - got)
    note(f"[ref order] config 3, 16 voices x 65,536 taps x 600 blocks: {n} of {ref.size} values differ (largest {worst:.2e} relative), "
         f"rms error {err:.2e}; bus rms {G.rms(ref):.4f}")
    assert n <= ref.size * 1e-4, n
    assert np.abs(ref - got).max() <= 2.0 ** -23 * np.abs(ref).max()   # never more than one float32 step at the signal's level
    assert err <= 1e-9


def test_one_voice_65536_taps_in_three_calls():
    """No bus sum behind the convolver, state carried over two call boundaries: the few values that differ do so by less than one
    float32 step at the signal's level (a flipped spectrum value is one step of ITS magnitude; where the 512 products cancel, the
    sum is small and the same absolute difference is several steps of the sum)."""
    frames = 128 * 600
    ref, got, st = render_pair(lambda c: G.config3_convolver(c, voices=1, taps=65536, frames=frames, ir_channels=1), frames,
                               pieces=[128 * 250, 128 * 100], conv_reference_order=2)
    assert st["ref_order_rows"] > 0
    n = int((ref != got).sum())
    step = 2.0 ** -23 * float(np.abs(ref).max())
    worst = float(np.abs(ref - got).max())
    note(f"[ref order] one voice x 65,536 taps x 600 blocks in three calls: {n} of {ref.size} values differ, largest difference "
         f"{worst / step:.3f} float32 steps at the signal's level")
    assert n <= ref.size * 1e-4 and worst <= step, (n, worst / step)


@pytest.mark.parametrize("taps", [1, 100, 128, 129, 300, 640, 8192, 8193, 128 * 70 + 5])
def test_tap_counts_bit_equal(taps):
    frames = 128 * 90
    ref, got, st = render_pair(lambda c: G.config3_convolver(c, voices=3, taps=taps, frames=frames), frames,
                               pieces=[128 * 7 + 3, 128 * 30, 128 * 11 + 70], conv_reference_order=2, max_chunk_blocks=37)
    assert st["ref_order_rows"] > 0
    if taps <= 640:   # few products per spectrum value: a flipped cast (see above) practically never shows
        assert np.array_equal(ref, got), flips(ref, got)
    else:
        assert (ref != got).sum() <= max(1, ref.size * 1e-4) and np.abs(ref - got).max() <= 2.0 ** -23 * np.abs(ref).max(), flips(ref, got)


def test_more_than_1024_partitions_two_tap_segments():
    frames = 128 * 60
    taps = 128 * 1100 + 17
    ref, got, st = render_pair(lambda c: G.config3_convolver(c, voices=2, taps=taps, frames=frames, ir_channels=1), frames,
                               pieces=[128 * 25], conv_reference_order=2)
    assert st["ref_order_rows"] > 0
    assert (ref != got).sum() <= ref.size * 1e-4 and np.abs(ref - got).max() <= 2.0 ** -23 * np.abs(ref).max(), flips(ref, got)


def test_true_stereo_and_private_impulse_responses_bit_equal():
    frames = 128 * 80

    def scene(ctx):
        ctx.Destination.SetChannelCount(2)
        for v in range(3):
            s = AudioBufferSourceNode(ctx)
            s.Buffer = PlayableAudioBuffer.FromChannelArrays([G.voice(10 * v, frames), G.voice(10 * v + 1, frames)], SR)
            cv = ConvolverNode(ctx)
            cv.Buffer = PlayableAudioBuffer.FromChannelArrays([G.synth_ir(c, 700 + 4000 * v, seed0=50 + 10 * v) for c in range(4)], SR)
            s.Connect(cv).Connect(ctx.Destination)
            s.Start(0.01 * v)
        return 2
    ref, got, st = render_pair(scene, frames, pieces=[128 * 33, 128 * 9], conv_reference_order=2)
    assert st["ref_order_rows"] > 0
    assert np.array_equal(ref, got), flips(ref, got)


def _sensitive_scene(kind):
    def scene(ctx):
        frames = 128 * 120
        ctx.Destination.SetChannelCount(2)
        s = AudioBufferSourceNode(ctx)
        s.Buffer = PlayableAudioBuffer.FromMonoArray(G.voice(5, frames), SR)
        cv = ConvolverNode(ctx)
        cv.Buffer = PlayableAudioBuffer.FromChannelArrays([G.synth_ir(c, 9000) for c in range(2)], SR)
        s.Connect(cv)
        s.Start()
        if kind == "resonant_biquad":       # fuzz graph 22879: a peaking filter at 104 Hz, Q 2.1 behind a convolver (2.6e-5 in round 3)
            bq = BiQuadFilterNode(ctx)
            bq.Type = FilterType.Peaking
            bq.Frequency.Value = 104.0
            bq.Q.Value = 2.1
            bq.Gain.Value = 6.0
            cv.Connect(bq).Connect(ctx.Destination)
        elif kind == "delay_time":          # fuzz graph 40542: (int)(delayTime * sampleRate) of a convolver-derived signal (5.7e-5)
            v = AudioBufferSourceNode(ctx)
            v.Buffer = PlayableAudioBuffer.FromMonoArray(G.voice(6, frames), SR)
            d = DelayNode(ctx, 0.05)
            d.DelayTime.Value = 0.004
            depth = GainNode(ctx)
            depth.Gain.Value = 0.02
            cv.Connect(depth)
            depth.Connect(d.DelayTime)
            v.Connect(d).Connect(ctx.Destination)
            v.Start()
        elif kind == "benign":              # a gain and a gentle low-pass: nothing that amplifies the last bit
            bq = BiQuadFilterNode(ctx)
            bq.Type = FilterType.Lowpass
            bq.Frequency.Value = 4000.0
            bq.Q.Value = 0.7
            g = GainNode(ctx)
            g.Gain.Value = 0.5
            cv.Connect(bq).Connect(g).Connect(ctx.Destination)
        return 2
    return scene


@pytest.mark.parametrize("kind", ["resonant_biquad", "delay_time"])
@pytest.mark.parametrize("coarse_forced", [0, 1])
def test_planner_takes_the_reference_order_where_the_last_bit_matters(kind, coarse_forced):
    """Default options: the convolver would take formulation C (short chunks) or D (coarse_min_blocks = 1); what sits behind it
    makes the planner choose R, and the render matches the oracle where round 3 documented 2.6e-5 / 5.7e-5."""
    frames = 128 * 120
    opts = {"coarse_min_blocks": 1} if coarse_forced else {}
    ref, got, st = render_pair(_sensitive_scene(kind), frames, pieces=[128 * 50, 128 * 31], **opts)
    assert st["ref_order_rows"] > 0 and st["stage_launches"][5] == 0
    n, worst = flips(ref, got)
    assert n <= ref.size * 1e-4 and G.rms(ref - got) <= 1e-7, (n, worst, G.rms(ref - got))
    # and with the route switched off the deviation of round 3 is back (the test would not notice a planner that never chooses R otherwise)
    ref2, got2, st2 = render_pair(_sensitive_scene(kind), frames, pieces=[128 * 50, 128 * 31], conv_reference_order=0, **opts)
    assert st2["ref_order_rows"] == 0
    assert G.rms(ref2 - got2) > 20 * max(G.rms(ref - got), 1e-9)


def test_planner_leaves_benign_graphs_and_the_headline_graph_alone():
    frames = 128 * 120
    ref, got, st = render_pair(_sensitive_scene("benign"), frames, coarse_min_blocks=1)
    assert st["ref_order_rows"] == 0 and st["stage_launches"][5] > 0
    assert G.rms(ref - got) <= 1e-5
    ref, got, st = render_pair(lambda c: G.config3_convolver(c, voices=32, taps=16384, frames=128 * 300), 128 * 300)
    assert st["ref_order_rows"] == 0 and st["stage_launches"][5] > 0 and st["coarse_premixed_signals"] > 0
    assert G.rms(ref - got) <= 1e-5


def test_a_convolver_moves_between_the_routes_when_its_consumers_change():
    """The decision is taken per chunk for convolvers on the B / C state layout (which R shares): a resonant biquad is connected
    behind a running convolver, and taken away again."""
    frames = 128 * 90
    outs, rows = [], []
    for device, ctx in enumerate((OracleContext(SR), OfflineAudioContext(SR))):
        ctx.Destination.SetChannelCount(2)
        s = AudioBufferSourceNode(ctx)
        s.Buffer = PlayableAudioBuffer.FromMonoArray(G.voice(5, frames), SR)
        cv = ConvolverNode(ctx)
        cv.Buffer = PlayableAudioBuffer.FromChannelArrays([G.synth_ir(c, 9000) for c in range(2)], SR)
        s.Connect(cv).Connect(ctx.Destination)
        s.Start()
        out = np.zeros((2, frames), np.float32)
        ctx.Render(out, 128 * 30, 0)
        bq = BiQuadFilterNode(ctx)
        bq.Type = FilterType.Peaking
        bq.Frequency.Value = 90.0
        bq.Q.Value = 2.5
        bq.Gain.Value = 6.0
        cv.Connect(bq).Connect(ctx.Destination)
        ctx.Render(out, 128 * 30, 128 * 30)
        if device:
            rows.append(ctx.GetStats()["ref_order_rows"])
        bq.Disconnect()
        ctx.Render(out, 128 * 30, 128 * 60)
        if device:
            rows.append(ctx.GetStats()["ref_order_rows"])
        outs.append(out)
        ctx.Dispose()
    assert rows[0] > 0 and rows[1] == rows[0]   # R while the biquad listens, back to C afterwards
    assert G.rms(outs[0] - outs[1]) <= 2e-6, G.rms(outs[0] - outs[1])
