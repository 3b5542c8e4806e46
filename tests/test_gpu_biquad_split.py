"""Constant-coefficient biquad cascades split along time (option biquad_time_split; ga_kernels.hpp, BiquadScanJob).

A long segment of a cascade is cut into pieces that run in parallel: pass A finds every piece's zero-state end state, a scan
chains them with A^K (float64, host), pass B runs every piece from its true initial state.  Every pass is the reference's
per-sample float arithmetic (BiQuadFilterNode.cs:137-138); what differs from the one-walk evaluation (option 0: bit-exact with the
oracle) is the rounding of the pieces' initial states.  These tests measure that difference against the oracle for the filters of
configs 2 and 4 and for the hard cases of a direct-form-II recursion (low cut-off, high Q, high-pass: large internal state,
cancelling output taps); their tolerances (1e-3 of the bus, 1e-5) only show a hand-over error of order one.  How close the split
is to float64 is measured on the scalar model of the path (tests/biquad_split_main.cpp, which the kernels equal bit for bit,
tests/test_gpu_biquad_split_kernels.py): over the cascades that mode 1 splits it is within 1.09 x the one walk's distance from
float64 and within 0.87 x the predicted deviation -- with A^K read as float64; rounded to float, as it was, the figures were 2.05 x
and 1.22 x.  Outside mode 1's threshold (forced mode 2) the prediction is not a bound and was never meant as one.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from graphaudio_amd import AudioBufferSourceNode, BiQuadFilterNode, FilterType, GainNode, OfflineAudioContext, PlayableAudioBuffer
from tests import _graphs as G
from tests._oracle import OracleContext
from tests._report import note

SR = 48000


def _render(mk, build, frames, pieces=None, **opts):
    ctx = mk(SR)
    for k, v in opts.items():
        ctx.SetOption(k, v)
    ch = build(ctx)
    out = np.zeros((ch, frames), np.float32)
    pos = 0
    for n in (pieces or [frames]):
        ctx.Render(out, n, pos)
        pos += n
    st = ctx.GetStats() if mk is OfflineAudioContext else None
    ctx.Dispose()
    return out, st


def test_config2_split_against_the_oracle_and_bit_exact_without():
    frames = 128 * 375
    build = lambda c: G.config2_biquad(c, voices=256, frames=frames)
    ref, _ = _render(OracleContext, build, frames)
    one, st1 = _render(OfflineAudioContext, build, frames, biquad_time_split=0)
    got, st = _render(OfflineAudioContext, build, frames)
    assert np.array_equal(ref, one) and st1["biquad_split_cascades"] == 0
    assert st["biquad_split_cascades"] == 256    # default mode: every one of these low-passes is inside the predicted-deviation bound
    err, sig = G.rms(ref - got), G.rms(ref)
    note(f"[biquad split] config 2, 256 voices: {st['biquad_split_cascades']} cascades split; bus rms {sig:.4f}, vs oracle abs rms {err:.3e} "
          f"(relative {err / sig:.3e})")
    assert err <= 1e-6 and err / sig < 2e-6


def test_config4_equaliser_is_not_split_by_default_and_why():
    """the 100 Hz low shelf of config 4 carries ~1e-4 of float32 rounding noise in the REFERENCE'S OWN direct-form-II arithmetic (large
    W, cancelling output taps): a different rounding cannot stay within 1e-5 of it once thousands of voices add up.  The default
    mode predicts that (Context::biquadDeviation) and keeps the one walk; mode 2 splits anyway and lands as far from the oracle as
    the oracle is from float64 truth."""
    frames = 128 * 375
    voices = 64
    build = lambda c: G.config4_eq(c, voices=voices, frames=frames)
    ref, _ = _render(OracleContext, build, frames)
    got, st = _render(OfflineAudioContext, build, frames)
    assert st["biquad_split_cascades"] == 0
    assert G.rms(ref - got) <= 1e-6 * max(G.rms(ref), 1e-3)
    forced, st2 = _render(OfflineAudioContext, build, frames, biquad_time_split=2)
    assert st2["biquad_split_cascades"] > 0
    err, sig = G.rms(ref - forced), G.rms(ref)
    note(f"[biquad split] config 4, {voices} voices x 5 sections, split forced: bus rms {sig:.4f}, vs oracle abs rms {err:.3e} (relative {err / sig:.3e})")
    assert err / sig < 1e-3   # noise level of the arithmetic, not an error of the split (next test: measured against float64)


HARD = [
    (FilterType.Lowpass, 40.0, 0.707, 0.0), (FilterType.Lowpass, 200.0, 10.0, 0.0), (FilterType.Highpass, 30.0, 0.707, 0.0),
    (FilterType.Highpass, 80.0, 10.0, 0.0), (FilterType.Bandpass, 60.0, 8.0, 0.0), (FilterType.Notch, 50.0, 10.0, 0.0),
    (FilterType.Peaking, 100.0, 10.0, 12.0), (FilterType.Lowshelf, 60.0, 1.0, -12.0), (FilterType.Highshelf, 12000.0, 1.0, 9.0),
    (FilterType.Allpass, 300.0, 5.0, 0.0),
]


def test_hard_filters_default_mode_stays_with_the_oracle_forced_mode_stays_at_noise_level():
    """(A float64 model cannot referee here: at these cut-offs one ulp of cosf moves the poles by a fraction of a per cent, so the
    reference's output depends on its libm to ~1e-2 -- SURVEY.md 8c.  What can be checked: the default mode only splits what it
    predicts to be harmless and then agrees with the oracle to 1e-5; forced, the split differs from the oracle by the rounding-noise
    level of the arithmetic, orders of magnitude below anything a state hand-over bug would produce.)"""
    frames = 128 * 1500   # 4 s: many pieces, long enough for the slowest poles
    x = [G.voice(300 + i, frames) for i in range(len(HARD))]

    def build(ctx):
        ctx.Destination.SetChannelCount(1)
        for i, (ft, f, q, g) in enumerate(HARD):
            s = AudioBufferSourceNode(ctx)
            s.Buffer = PlayableAudioBuffer.FromMonoArray(x[i], SR)
            bq = BiQuadFilterNode(ctx)
            bq.Type = ft
            bq.Frequency.Value = f
            bq.Q.Value = q
            bq.Gain.Value = g
            bq.Inputs[0].SetChannelCount(1)
            gn = GainNode(ctx)
            gn.Inputs[0].SetChannelCount(1)
            gn.Gain.Value = 1.0
            s.Connect(bq).Connect(gn).Connect(ctx.Destination)
            s.Start()
        return 1

    ref, _ = _render(OracleContext, build, frames)
    auto, st_auto = _render(OfflineAudioContext, build, frames)
    forced, st = _render(OfflineAudioContext, build, frames, biquad_time_split=2)
    assert st["biquad_split_cascades"] == len(HARD)
    sig = G.rms(ref)
    note(f"[biquad split] hard filters: bus rms {sig:.4f}; default mode splits {st_auto['biquad_split_cascades']} of {len(HARD)}: vs oracle "
          f"{G.rms(ref - auto):.3e}; forced: vs oracle {G.rms(ref - forced):.3e}")
    assert 0 < st_auto["biquad_split_cascades"] < len(HARD)
    assert G.rms(ref - auto) <= 1e-5
    assert G.rms(ref - forced) <= 1e-3 * sig


def test_cascades_and_stereo_in_uneven_pieces():
    """5-section cascades on stereo signals, rendered in pieces around the split threshold: state hand-over piece -> scan -> piece
    -> next render call"""
    frames = 128 * 900

    def build(ctx):
        G.config4_eq(ctx, voices=6, frames=frames)
        return 2

    ref, _ = _render(OracleContext, build, frames)
    got, st = _render(OfflineAudioContext, build, frames, pieces=[128 * 130, 128 * 300, 128 * 20, 128 * 450], biquad_time_split=2)
    assert st["biquad_split_cascades"] > 0
    err, sig = G.rms(ref - got), G.rms(ref)
    assert err / sig < 1e-3, (err, sig)   # (rounding-noise level of these low-frequency sections; a hand-over bug would be O(1))
    # ... and a well-conditioned cascade (two mid-band sections per voice) under the default mode, same pieces
    def build2(ctx):
        ctx.Destination.SetChannelCount(2)
        for v in range(6):
            s = AudioBufferSourceNode(ctx)
            s.Buffer = PlayableAudioBuffer.FromStereoArrays(G.voice(2 * v, frames), G.voice(2 * v + 1, frames), SR)
            node = s
            for f in (1500.0 + 300 * v, 5000.0):
                bq = BiQuadFilterNode(ctx)
                bq.Type = FilterType.Peaking
                bq.Frequency.Value = f
                bq.Q.Value = 1.0
                bq.Gain.Value = 5.0
                node = node.Connect(bq)
            node.Connect(ctx.Destination)
            s.Start()
        return 2
    ref2, _ = _render(OracleContext, build2, frames)
    got2, st2 = _render(OfflineAudioContext, build2, frames, pieces=[128 * 130, 128 * 300, 128 * 20, 128 * 450])
    assert st2["biquad_split_cascades"] > 0
    assert G.rms(ref2 - got2) <= 2e-6 * G.rms(ref2)
