"""Option "ir_resample" through the Python host ("Impulse responses at another sample rate"): an impulse response
or an HRIR set at another sample rate than the context's is converted once, at assignment, on the device.

The truth is the float64 model tests/_ir_resample_model.py: the converted buffer np.float32(model) at 48 kHz, given to the CPU oracle
(convolvers) or to the same kind of context (HRIR sets; the oracle has no SpatialPannerNode).  Bounds are those of the tests the
scenes come from: tests/test_gpu_parity.py::test_convolver_small (rms error <= 1e-5 and <= 2e-6 x max(rms(ref), 1e-3)) and
tests/test_gpu_spatial.py::check (max-abs <= 1e-5 x max(1, peak)).

test_a_delta_keeps_a_sine is the test of the fi / fo rule, independent of the model's gain.  The request for this option worded
the case as "a [1.0] IR".  By the definition (M = (N L + D - 1) / D, terms outside the row skipped) a one-frame buffer converts to
two frames -- the kernel cut off at its centre -- which is no identity for any input.  The case is therefore the one-sample impulse
with W + 1 frames of silence on either side, which the definition converts to the whole kernel; everything else (the 1 kHz sine,
Normalize off, the 1e-5 bound -- the passband bound of 1e-6 with its margin --, the group delay) is as requested, and the frames
compared are those behind the converted response's own length (154 frames) instead of behind 2W = 138.
"""
import math
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from graphaudio_amd import (AudioBufferSourceNode, ConvolverNode, HrirSet, InvalidOperationException, NotSupportedException,
                            OfflineAudioContext, PlayableAudioBuffer, SpatialPannerNode)
from graphaudio_amd import ArgumentException, ArgumentOutOfRangeException
from graphaudio_amd.io import AudioDecoder
from tests import _graphs as G
from tests import _ir_resample_model as model
from tests._oracle import OracleContext

SR = 48000
B = 128
FRAMES = 48 * B
TOL_RMS = 1e-5


def convolver_graph(ctx, irs, ir_sr, normalize=True, voices=3, frames=FRAMES, irbuf=None):
    """voices -> per-voice ConvolverNode on one impulse response -> destination"""
    irbuf = irbuf or PlayableAudioBuffer.FromChannelArrays(list(irs), ir_sr)
    out_ch = 2 if len(irs) == 4 else len(irs)
    ctx.Destination.SetChannelCount(out_ch)
    nodes = []
    for v in range(voices):
        s = AudioBufferSourceNode(ctx)
        s.Buffer = PlayableAudioBuffer.FromMonoArray(G.voice(v, frames + 256), SR)
        cv = ConvolverNode(ctx)
        cv.Normalize = normalize
        cv.Buffer = irbuf
        s.Connect(cv).Connect(ctx.Destination)
        s.Start()
        nodes.append((s, cv))
    return out_ch, nodes


def truth(irs, fi, normalize, **kw):
    o = OracleContext(SR)
    conv = [np.float32(model.resample(h, fi, SR)) for h in irs]
    ch, _ = convolver_graph(o, conv, SR, normalize, **kw)
    ref = G.render(o, ch, kw.get("frames", FRAMES))
    o.Dispose()
    return ref


def device(irs, fi, normalize, options=(), **kw):
    ctx = OfflineAudioContext(SR)
    ctx.SetOption("ir_resample", 1)
    for k, v in options:
        ctx.SetOption(k, v)
    ch, _ = convolver_graph(ctx, irs, fi, normalize, **kw)
    got = G.render(ctx, ch, kw.get("frames", FRAMES))
    st = ctx.GetStats()
    ctx.Dispose()
    return got, st


def compare(ref, got, what):
    err = G.rms(ref - got)
    print(f"{what}: rms(ref) {G.rms(ref):.4e}  rms error {err:.3e} = {err / max(G.rms(ref), 1e-3):.3e} x max(rms(ref), 1e-3)")
    assert G.rms(ref) > 1e-4
    assert err <= TOL_RMS, err
    assert err <= 2e-6 * max(G.rms(ref), 1e-3)


# ---- 1. option off: the reference's refusal -------------------------------------------------------------------------------------

def test_option_off_refuses_as_before():
    ctx = OfflineAudioContext(SR)
    cv = ConvolverNode(ctx)
    with pytest.raises(InvalidOperationException, match="Impulse response buffer sample rate must match the audio context sample rate."):
        cv.Buffer = PlayableAudioBuffer.FromMonoArray(G.synth_ir(0, 300), 44100)
    p = SpatialPannerNode(ctx)
    p.HrirAzimuths = 4
    hr = (np.random.default_rng(3).standard_normal((12, 2, 64)) * 0.1).astype(np.float32)
    with pytest.raises(InvalidOperationException, match="HRIR set sample rate must match the audio context sample rate."):
        p.Hrir = HrirSet.FromArray(hr, 44100)
    ctx.Dispose()


def test_option_values():
    ctx = OfflineAudioContext(SR)
    ctx.SetOption("ir_resample", 1)
    ctx.SetOption("ir_resample", 0)
    for bad in (2, -1, 0.5):
        with pytest.raises(ArgumentOutOfRangeException):
            ctx.SetOption("ir_resample", bad)
    cv = ConvolverNode(ctx)   # off again: refused again
    with pytest.raises(InvalidOperationException):
        cv.Buffer = PlayableAudioBuffer.FromMonoArray(G.synth_ir(0, 300), 44100)
    assert ctx.GetStats()["ir_resamples"] == 0
    ctx.Dispose()


# ---- 2 / 3. convolvers against the oracle on the model-converted impulse response -------------------------------------------------

@pytest.mark.parametrize("normalize", [True, False])
def test_mono_ir_at_44100(normalize):
    irs = [G.synth_ir(0, 300)]
    got, st = device(irs, 44100, normalize)
    assert st["ir_resamples"] == 1
    compare(truth(irs, 44100, normalize), got, f"mono 300 taps, Normalize {normalize}")


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("shape", ["true_stereo_96k", "stereo_9000_coarse", "one_tap", "five_taps"])
def test_other_shapes(shape, normalize):
    options = ()
    if shape == "true_stereo_96k":
        fi, irs = 96000, [G.synth_ir(c, 2000) for c in range(4)]
    elif shape == "stereo_9000_coarse":   # formulation D transforms the converted taps kept by the spectra
        fi, irs, options = 44100, [G.synth_ir(c, 9000) for c in range(2)], (("coarse_min_blocks", 1),)
    elif shape == "one_tap":              # N < W
        fi, irs = 44100, [np.array([0.75], np.float32)]
    else:
        fi, irs = 44100, [G.synth_ir(0, 5)]
    got, st = device(irs, fi, normalize, options)
    assert st["ir_resamples"] == 1
    if shape == "stereo_9000_coarse":
        assert st["stage_launches"][5] > 0 and st["stage_launches"][6] > 0
    compare(truth(irs, fi, normalize), got, f"{shape}, Normalize {normalize}")


# ---- 4. the fi / fo rule: a delta stays a band-limited identity -------------------------------------------------------------------

def test_a_delta_keeps_a_sine():
    fi = 44100
    p = model.plan(fi, SR)
    centre = p.W + 1
    ir = np.zeros(2 * centre + 1, np.float32)
    ir[centre] = 1.0
    m = model.out_length(ir.size, p)
    frames = 16 * B
    amp, f0 = 0.5, 1000.0
    n = np.arange(frames + 256)
    x = (amp * np.sin(2.0 * np.pi * f0 * n / SR)).astype(np.float32)
    ctx = OfflineAudioContext(SR)
    ctx.SetOption("ir_resample", 1)
    ctx.Destination.SetChannelCount(1)
    s = AudioBufferSourceNode(ctx)
    s.Buffer = PlayableAudioBuffer.FromMonoArray(x, SR)
    cv = ConvolverNode(ctx)
    cv.Normalize = False
    cv.Buffer = PlayableAudioBuffer.FromMonoArray(ir, fi)
    s.Connect(cv).Connect(ctx.Destination)
    s.Start()
    out = G.render(ctx, 1, frames)[0]
    ctx.Dispose()
    delay = centre * SR / fi                      # the impulse sits at centre / fi seconds: the converted filter's group delay, in 48 kHz frames
    k = np.arange(m, frames)
    want = amp * np.sin(2.0 * np.pi * f0 * (k - delay) / SR)
    err = float(np.max(np.abs(out[m:].astype(np.float64) - want)))
    print(f"delta at frame {centre} of {ir.size} -> {m} frames, group delay {delay:.4f} frames: max-abs error behind frame {m}: {err:.3e}")
    assert m == 154 and frames - m > 10 * SR / f0
    assert err <= 1e-5


# ---- 5. one conversion per buffer and context ---------------------------------------------------------------------------------------

def test_one_conversion_per_buffer():
    ctx = OfflineAudioContext(SR)
    ctx.SetOption("ir_resample", 1)
    irs = [G.synth_ir(0, 300)]
    irbuf = PlayableAudioBuffer.FromChannelArrays(irs, 44100)
    ch, nodes = convolver_graph(ctx, irs, 44100, irbuf=irbuf)
    assert ctx.GetStats()["ir_resamples"] == 1
    G.render(ctx, ch, 4 * B)
    cv = ConvolverNode(ctx)
    cv.Buffer = irbuf
    cv.Connect(ctx.Destination)
    other = ConvolverNode(ctx)
    other.Normalize = False      # (other spectra, the same converted taps)
    other.Buffer = irbuf
    assert ctx.GetStats()["ir_resamples"] == 1
    ctx.SetOption("ir_resample", 0)   # switching it off leaves the assignments alone
    out = np.zeros((ch, 4 * B), np.float32)
    ctx.Render(out, 4 * B, 0)
    assert G.rms(out) > 1e-4
    ctx.SetOption("ir_resample", 1)
    for _, c in nodes:
        c.Buffer = None
    cv.Buffer = None
    other.Buffer = None
    del irbuf                    # ga_buffer_release
    G.render(ctx, ch, 2 * B)
    cv.Buffer = PlayableAudioBuffer.FromChannelArrays(irs, 44100)
    assert ctx.GetStats()["ir_resamples"] == 2
    ctx.Dispose()


def _bytes_freed_by_release(rate, option):
    """device bytes that go when a buffer is released that one convolver used as its 300-tap impulse response"""
    ctx = OfflineAudioContext(SR)
    ctx.SetOption("ir_resample", option)
    irs = [G.synth_ir(0, 300)]
    irbuf = PlayableAudioBuffer.FromChannelArrays(irs, rate)
    bid = irbuf._native_id(ctx)
    ch, nodes = convolver_graph(ctx, irs, rate, voices=1, irbuf=irbuf)
    G.render(ctx, ch, 4 * B)
    nodes[0][1].Buffer = None
    G.render(ctx, ch, 2 * B)              # the queued swap is executed, the node's state released: the buffer is only held by its handle
    before = ctx.GetStats()["device_bytes_in_use"]
    ctx._call("buffer_release", bid)      # what PlayableAudioBuffer.__del__ does
    G.render(ctx, ch, 2 * B)              # released buffers go in front of the next chunk
    after = ctx.GetStats()["device_bytes_in_use"]
    n = ctx.GetStats()["ir_resamples"]
    irbuf._ids.clear()                    # (released by hand above)
    ctx.Dispose()
    return before - after, n


def test_a_released_buffer_takes_its_copy_along():
    """The same steps with a 44.1 kHz buffer (converted) and with a 48 kHz buffer of the same length: 300 and 327 taps are both 3
    partitions, so what is freed differs by the converted copy alone -- its rows of (327 + 8 rounded up to 64) floats plus the 64 KiB
    by which every buffer's allocation is skewed."""
    freed_44, n_44 = _bytes_freed_by_release(44100, 1)
    freed_48, n_48 = _bytes_freed_by_release(SR, 1)
    m = model.out_length(300, model.plan(44100, SR))
    copy = (m + 8 + 63) // 64 * 64 * 4 + 64 * 1024
    print(f"freed by the release: {freed_44} bytes with a converted copy, {freed_48} without; the copy is {copy} bytes")
    assert (n_44, n_48) == (1, 0) and m == 327
    assert freed_48 > 0
    assert freed_44 - freed_48 == copy


# ---- 6. a rate pair beyond the table cap ------------------------------------------------------------------------------------------

def test_rate_pair_beyond_the_table_cap_is_refused_and_the_context_lives():
    ctx = OfflineAudioContext(SR)
    ctx.SetOption("ir_resample", 1)
    cv = ConvolverNode(ctx)
    with pytest.raises(NotSupportedException, match="2\\^22"):
        cv.Buffer = PlayableAudioBuffer.FromMonoArray(G.synth_ir(0, 300), 44101)
    p = SpatialPannerNode(ctx)
    p.HrirAzimuths = 4
    hr = (np.random.default_rng(3).standard_normal((12, 2, 64)) * 0.1).astype(np.float32)
    with pytest.raises(NotSupportedException):
        p.Hrir = HrirSet.FromArray(hr, 44101)
    with pytest.raises(ArgumentException):   # the empty-buffer error stays
        cv.Buffer = PlayableAudioBuffer.FromMonoArray(np.zeros(0, np.float32), 44100)
    assert ctx.GetStats()["ir_resamples"] == 0
    irs =[G.synth_ir(c, 1000) for c in range(2)]
    ch, _ = convolver_graph(ctx, irs, SR)
    got = G.render(ctx, ch, FRAMES)
    ctx.Dispose()
    o = OracleContext(SR)
    convolver_graph(o, irs, SR)
    compare(G.render(o, ch, FRAMES), got, "a valid graph behind the refusal")


# ---- 7. an HRIR set at 44.1 kHz -------------------------------------------------------------------------------------------------

def spatial_scene(ctx, hrir, sr, frames):
    """a static source and one that crosses in front of the listener (every block fades)"""
    nodes = []
    for i, moving in enumerate((False, True)):
        s = AudioBufferSourceNode(ctx)
        s.Buffer = PlayableAudioBuffer.FromMonoArray(np.concatenate([G.voice(40 + i, frames), np.zeros(256, np.float32)]), SR)
        p = SpatialPannerNode(ctx)
        p.HrirAzimuths = 4
        p.Hrir = HrirSet.FromArray(hrir, sr)
        p.PositionY.Value = 0.4
        p.PositionZ.Value = -1.0
        if moving:
            p.PositionX.SetValueAtTime(-3.0, 0.0)
            p.PositionX.LinearRampToValueAtTime(3.0, frames / SR)
        else:
            p.PositionX.Value = 1.3
        s.Connect(p).Connect(ctx.Destination)
        s.Start()
        nodes.append((s, p))
    return nodes


def test_hrir_set_at_44100():
    frames = 20 * B
    k = np.arange(64)
    hrir = (np.random.default_rng(91).standard_normal((12, 2, 64)) * np.exp(-6.9 * k / 64) * 0.5).astype(np.float32)
    outs = []
    for converted in (False, True):
        ctx = OfflineAudioContext(SR)
        if converted:
            hold = spatial_scene(ctx, np.float32(model.resample(hrir, 44100, SR)), SR, frames)
        else:
            ctx.SetOption("ir_resample", 1)
            hold = spatial_scene(ctx, hrir, 44100, frames)
        out = np.zeros((2, frames), np.float32)
        ctx.Render(out, frames)
        assert ctx.GetStats()["ir_resamples"] == (0 if converted else 2)   # (two HrirSet objects: two buffers)
        ctx.Dispose()
        outs.append(out)
    got, ref = outs[0], outs[1].astype(np.float64)
    scale = max(1.0, float(np.max(np.abs(ref))))
    err = float(np.max(np.abs(got.astype(np.float64) - ref)))
    print(f"HRIR set 12 x 2 x 64 at 44.1 kHz: max-abs error {err:.3e} = {err / scale:.3e} x max(1, peak {float(np.max(np.abs(ref))):.3f})")
    assert G.rms(got) > 1e-3
    assert err <= 1e-5 * scale


def test_hrir_frame_limit_applies_to_the_converted_length():
    ctx = OfflineAudioContext(SR)
    ctx.SetOption("ir_resample", 1)
    p = SpatialPannerNode(ctx)
    p.HrirAzimuths = 1
    rng = np.random.default_rng(5)
    p.Hrir = HrirSet.FromArray((rng.standard_normal((1, 2, 470)) * 0.05).astype(np.float32), 44100)    # 512 frames at 48 kHz
    with pytest.raises(InvalidOperationException, match="471 frames at 44100 Hz are 513 frames at 48000 Hz"):
        p.Hrir = HrirSet.FromArray((rng.standard_normal((1, 2, 471)) * 0.05).astype(np.float32), 44100)
    with pytest.raises(InvalidOperationException, match="multiple of 2 \\* hrirAzimuths"):               # the channel rules are unchanged
        q = SpatialPannerNode(ctx)
        q.HrirAzimuths = 4
        q.Hrir = HrirSet.FromArray((rng.standard_normal((6, 2, 64)) * 0.05).astype(np.float32), 44100)
    s = AudioBufferSourceNode(ctx)
    s.Buffer = PlayableAudioBuffer.FromMonoArray(G.voice(3, 6 * B + 256), SR)
    p.PositionX.Value = 1.0
    s.Connect(p).Connect(ctx.Destination)
    s.Start()
    out = np.zeros((2, 6 * B), np.float32)
    ctx.Render(out, 6 * B)
    assert G.rms(out) > 1e-4 and np.isfinite(out).all()
    ctx.Dispose()


# ---- 8. a 44.1 kHz WAV file -----------------------------------------------------------------------------------------------------

def test_wav_file_at_44100_into_a_convolver(tmp_path):
    pcm = np.clip(np.round(G.synth_ir(0, 300) * 0.25 * 32768.0), -32768, 32767).astype("<i2")
    path = str(tmp_path / "ir.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(44100)
        w.writeframes(pcm.tobytes())
    buf = AudioDecoder.LoadFromFile(path)
    # (the frame count comes from the Duration in whole 100 ns ticks, as in the reference's loader: 300 frames at 44.1 kHz are 299)
    assert buf.SampleRate == 44100 and buf.NumberOfChannels == 1 and buf.Length in (299, 300)
    taps = buf.GetChannelData(0)
    assert np.array_equal(taps, (pcm.astype(np.float32) / np.float32(32768.0))[:buf.Length])
    ctx = OfflineAudioContext(SR)
    ctx.SetOption("ir_resample", 1)
    ch, _ = convolver_graph(ctx, [taps], 44100, irbuf=buf)
    got = G.render(ctx, ch, FRAMES)
    assert ctx.GetStats()["ir_resamples"] == 1
    ctx.Dispose()
    compare(truth([taps], 44100, True), got, "16-bit WAV at 44.1 kHz")


# ---- 9. conversion happens at assignment, not per chunk -------------------------------------------------------------------------

def _in_pieces(ctx, ch):
    got = np.zeros((ch, FRAMES), np.float32)
    pos = 0
    for piece in (100, 391, 1, FRAMES):
        k = min(piece, FRAMES - pos)
        if k > 0:
            ctx.Render(got, k, pos)
            pos += k
    assert pos == FRAMES
    return got


def test_uneven_pieces_and_one_piece():
    """The same output, value for value, however the render is cut: the response is converted when it is assigned (ir_resamples
    stays 1), and the convolver that then runs is the one a response at the context's rate gets, which this scene (3 partitions,
    the per-block formulations) renders the same in pieces and in one piece -- shown beside it with the model-converted response."""
    irs = [G.synth_ir(0, 300)]
    ref = truth(irs, 44100, True)
    whole, _ = device(irs, 44100, True)
    ctx = OfflineAudioContext(SR)
    ctx.SetOption("ir_resample", 1)
    ch, _ = convolver_graph(ctx, irs, 44100)
    got = _in_pieces(ctx, ch)
    assert ctx.GetStats()["ir_resamples"] == 1
    ctx.Dispose()
    compare(ref, got, "pieces 100, 391, 1, rest")
    native = [np.float32(model.resample(h, 44100, SR)) for h in irs]
    outs = []
    for pieces in (False, True):
        ctx = OfflineAudioContext(SR)
        ch, _ = convolver_graph(ctx, native, SR)
        outs.append(_in_pieces(ctx, ch) if pieces else G.render(ctx, ch, FRAMES))
        ctx.Dispose()
    print(f"pieces against one piece: rms difference {G.rms(got - whole):.3e}, {int((got != whole).sum())} of {got.size} values differ; "
          f"with the model-converted response at 48 kHz: {int((outs[0] != outs[1]).sum())} differ")
    assert np.array_equal(got, whole)
