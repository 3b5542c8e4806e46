"""Edges of a signal-modulated playbackRate (two-stage chunks: DESIGN.md "Modulated playbackRate"): loop regions inside the buffer,
loops shorter than a block, Start(when, offset, duration) and Stop(t), a source that resumes after an END block, buffers of more than
one channel, the copy path at a non-unit buffer ratio, and more than 64 modulated sources with different geometry.  The HIP path
against the CPU oracle, rendered as one piece and in uneven pieces of short chunks; the device walk against the host replay.  Every
case first checks on the oracle's output that the edge it targets happens.  Last: non-finite modulation of gain / pan / offset
(Math.Clamp keeps a NaN)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from graphaudio_amd import (AudioBufferSourceNode, ConstantSourceNode, GainNode, NotSupportedException, OfflineAudioContext,
                            OscillatorNode, PlayableAudioBuffer, StereoPannerNode)
from tests import _graphs as G
from tests._oracle import OracleContext
from tests.test_gpu_playback_rate_mod import SR, _lfo, _refused_then_supported, pair, render

B = 128
FORMS = {"default": (None, None), "chunk5": ([1000, 777, 128 * 9 + 5, 3001], {"max_chunk_blocks": 5})}


def both(build, frames, form, ch=2):
    pieces, opts = FORMS[form]
    return pair(build, ch, frames, pieces=pieces, opts=opts)


def walk_vs_host(build, frames, chunk=5):
    walk = render(OfflineAudioContext, build, 2, frames, opts={"rate_mod_walk": 1, "max_chunk_blocks": chunk})
    host = render(OfflineAudioContext, build, 2, frames, opts={"rate_mod_walk": 0, "max_chunk_blocks": chunk})
    assert G.rms(walk) > 1e-3
    assert np.array_equal(walk, host)


def region_buffer(seed, n, a, b, nch=1, before=0.0):
    """Noise in frames [a, b), `before` times noise in front of a, silence from b on: sound after the first pass to b proves the
    loop wrapped."""
    chans = []
    for c in range(nch):
        x = G.voice(seed + 17 * c, n)
        x[:a] *= before
        x[b:] = 0.0
        chans.append(x)
    return chans


def src(ctx, chans, sr, loop=True, ls=None, le=None):
    s = AudioBufferSourceNode(ctx)
    s.Buffer = PlayableAudioBuffer.FromChannelArrays(chans, sr)
    s.Loop = loop
    if ls is not None:
        s.LoopStart = (ls + 0.5) / sr   # (int)(LoopStart * sampleRate) lands on frame ls
    if le is not None:
        s.LoopEnd = (le + 0.5) / sr if le > 0 else 0.0
    return s


def timeline(ctx, param, points):
    """A ConstantSourceNode whose offset steps through (time, value) points, added to `param`."""
    cs = ConstantSourceNode(ctx)
    cs.Offset.SetValueAtTime(0.0, 0.0)
    for t, v in points:
        cs.Offset.SetValueAtTime(v, t)
    cs.Connect(param)
    cs.Start()
    return cs


def tail_sounds(out, blocks=8):
    return G.rms(out[:, -B * blocks:]) > 1e-3


# ---- 1. loop regions inside the buffer ------------------------------------------------------------------------------------------

# (name, buffer rate, buffer length, loopStart frame, loopEnd frame (0: unset), sound in front of the region)
REGIONS = [
    ("inside_441", 44100, 30000, 1234, 3877, 0.0),
    ("inside_2205", 22050, 20000, 777, 2321, 0.0),
    ("after_position", 44100, 30000, 5003, 6999, 0.5),   # the region starts after the playback position: one pass from 0 first
    ("end_clamped", 44100, 4000, 2001, 50000, 0.0),      # LoopEnd past the buffer's end: clamped to the length
    ("end_unset", 44100, 3000, 0, 0, 0.0),               # LoopEnd = 0: the whole buffer
]
FRAMES_REGION = B * 150


def region_case(sr, n, ls, le, before):
    def build(ctx):
        chans = region_buffer(11, n, ls, le if 0 < le < n else n, before=before)
        s = src(ctx, chans, sr, ls=ls, le=le)
        hold = _lfo(ctx, 6.0, 0.2, s.PlaybackRate)
        s.Connect(ctx.Destination)
        s.Start()
        return (s,) + hold
    return build


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name,sr,n,ls,le,before", REGIONS)
def test_loop_region(name, sr, n, ls, le, before, form):
    ref, got = both(region_case(sr, n, ls, le, before), FRAMES_REGION, form)
    # the edge: the rate stays >= 0.8, so the source consumes >= 0.8 * ratio * frames; that is several loop lengths past the
    # region's end, and the buffer is silent outside the region: sound in the last blocks means the loop wrapped
    end = le if 0 < le < n else n
    consumed = 0.8 * sr / SR * FRAMES_REGION
    assert (consumed - end) / (end - ls) >= 2.0
    assert tail_sounds(ref)
    if before:
        assert G.rms(ref[:, :B * 4]) > 1e-3
    assert np.array_equal(ref, got)


def fast_loop(ctx):
    """A 1,000-frame loop at rates ramped from 1 up to 60 and back: at a few times the block length the wrap buffer stops short of
    the block's end (the block keeps fewer than 128 samples), where the 4 samples of the `needed` margin decide the count."""
    chans = region_buffer(12, 3000, 500, 1500)
    s = src(ctx, chans, SR, ls=500, le=1500)
    s.PlaybackRate.SetValueAtTime(1.0, 0.0)
    s.PlaybackRate.LinearRampToValueAtTime(60.0, 0.15)
    s.PlaybackRate.LinearRampToValueAtTime(1.0, 0.3)
    hold = _lfo(ctx, 9.0, 0.3, s.PlaybackRate)
    s.Connect(ctx.Destination)
    s.Start()
    return (s,) + hold


@pytest.mark.parametrize("form", list(FORMS))
def test_fast_rates_on_a_loop(form):
    ref, got = both(fast_loop, B * 120, form)
    # the edge: blocks that end in zeros (the wrap buffer could not feed the rate) between sounding ones
    short = [b for b in range(120) if np.any(ref[0, b * B:(b + 1) * B] != 0) and np.all(ref[0, (b + 1) * B - 8:(b + 1) * B] == 0)]
    assert len(short) >= 5, short
    assert tail_sounds(ref)
    assert np.array_equal(ref, got)


# ---- 2. loops shorter than a block: the wrap buffer in every block ------------------------------------------------------------

SHORT = [1, 3, 4, 5, 127, 128, 129]


def short_case(length, sr=44100):
    def build(ctx):
        ls = 301
        chans = region_buffer(13 + length, 1200, ls, ls + length)
        s = src(ctx, chans, sr, ls=ls, le=ls + length)
        hold = _lfo(ctx, 5.0, 0.4, s.PlaybackRate)
        s.Connect(ctx.Destination)
        s.Start(0.0, 290.5 / sr)   # (offset: 11 frames in front of the loop)
        return (s,) + hold
    return build


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("length", SHORT)
def test_short_loop(length, form):
    frames = B * 100
    ref, got = both(short_case(length), frames, form)
    # the edge: the buffer is silent outside the loop; the source ran >= 0.6 * ratio * frames past it, many loop lengths
    assert 0.6 * 44100 / SR * frames / length > 40
    assert tail_sounds(ref)
    assert np.array_equal(ref, got)


# ---- 3. a zero-length loop under modulation: refused before anything moves --------------------------------------------------

def test_zero_length_loop_refused_then_fixed():
    def make(ctx):
        chans = region_buffer(14, 8000, 0, 8000)
        s = src(ctx, chans, 44100, ls=3000, le=3000)   # LoopStart >= LoopEnd
        hold = _lfo(ctx, 5.0, 0.1, s.PlaybackRate)
        s.Connect(ctx.Destination)
        s.Start()

        def fix():
            s.LoopEnd = 5000.5 / 44100
        return (s,) + hold, fix
    _refused_then_supported(make)


# ---- 4. Start(when, offset, duration) -------------------------------------------------------------------------------------------

def start_case(kind):
    def build(ctx):
        if kind == "offset":        # looping from an offset into the buffer, no duration
            s = src(ctx, region_buffer(15, 20000, 0, 20000), 44100, ls=4000, le=16000)
            s.Start(0.013, 6000.5 / 44100)
        elif kind == "duration":    # a stop time mid-chunk: the walk goes on past the END block (endsAtEnd = 0)
            s = src(ctx, region_buffer(16, 40000, 0, 40000), 44100, loop=False)
            s.Start(0.007, 1000.5 / 44100, (B * 41 + 50) / SR)
        else:                       # the same duration, but the one-shot's data runs out before durEnd
            s = src(ctx, region_buffer(17, 4000, 0, 4000), 44100, loop=False)
            s.Start(0.007, 1000.5 / 44100, (B * 41 + 50) / SR)
        hold = _lfo(ctx, 4.0, 0.3, s.PlaybackRate)
        s.Connect(ctx.Destination)
        return (s,) + hold
    return build


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("kind", ["offset", "duration", "data_runs_out"])
def test_start_offset_duration(kind, form):
    frames = B * 90
    ref, got = both(start_case(kind), frames, form)
    start = int(0.007 * SR) // B
    blocks = [G.rms(ref[:, b * B:(b + 1) * B]) for b in range(frames // B)]
    if kind == "offset":
        assert tail_sounds(ref) and blocks[0] == 0.0 and blocks[5] > 0
    else:
        # the edge: sound, then silence from the first END block on.  "duration": the source consumes the 4,867 frames up to
        # durEnd (offset + duration) at a rate above 1 on average and goes silent there, well before the stop time (block 44);
        # "data_runs_out": the 3,000 frames of data behind the offset run out before durEnd
        last = max(b for b in range(len(blocks)) if blocks[b] > 0)
        assert blocks[start + 2] > 0 and all(v == 0.0 for v in blocks[last + 1:])
        if kind == "duration":
            assert start + 25 < last < 43
        else:
            assert last < start + 25
    assert np.array_equal(ref, got)


# ---- 5. Stop(t) under modulation ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("stop_block", [3, 9, 27])   # (chunk5: before, inside and after the chunk that holds t)
def test_stop_under_modulation(stop_block, form):
    t = (stop_block * B + 37) / SR

    def build(ctx):
        s = src(ctx, region_buffer(18, 9000, 0, 9000), 44100, ls=1000, le=7000)
        hold = _lfo(ctx, 7.0, 0.25, s.PlaybackRate)
        s.Connect(ctx.Destination)
        s.Start()
        s.Stop(t)
        return (s,) + hold
    frames = B * 60
    ref, got = both(build, frames, form)
    # the edge: sound up to the block that holds t, silence from the next one on
    assert G.rms(ref[:, stop_block * B:(stop_block + 1) * B]) > 0 and not ref[:, (stop_block + 1) * B:].any()
    assert np.array_equal(ref, got)


# ---- 6. an END block, then audio again (a stop time is set) ----------------------------------------------------------------------

def resumes(ctx):
    """A looping source with a late stop time; a ConstantSourceNode drives the rate to 1000 for a few blocks (the wrap buffer cannot
    feed it: END blocks) and then back to exactly 1 (the copy path: the resampler's stale position does not hold it back)."""
    s = src(ctx, region_buffer(19, 10000, 0, 10000), SR, ls=100, le=9000)
    cs = timeline(ctx, s.PlaybackRate, [(B * 10 / SR, 999.0), (B * 15 / SR, 0.0)])
    s.Connect(ctx.Destination)
    s.Start()
    s.Stop(B * 70 / SR)
    return (s, cs)


def test_end_then_audio_again_one_block_chunks():
    frames = B * 40
    ref = render(OracleContext, resumes, 2, frames)
    got = render(OfflineAudioContext, resumes, 2, frames, opts={"max_chunk_blocks": 1})
    blocks = [G.rms(ref[:, b * B:(b + 1) * B]) for b in range(frames // B)]
    # the edge: a silent (END) block between sounding ones
    assert any(blocks[b] > 0 and blocks[b + 1] == 0 for b in range(8, 16))
    assert any(blocks[b] == 0 and blocks[b + 1] > 0 for b in range(8, 20))
    assert tail_sounds(ref)
    assert np.array_equal(ref, got)


def test_end_then_audio_again_in_one_chunk_is_refused():
    """In one chunk the device walk sees the END block and the audio after it: it refuses (GSR_ERR_RESUMED) instead of rendering
    different audio -- this is what the code does today."""
    ctx = OfflineAudioContext(SR)
    ctx.Destination.SetChannelCount(2)
    hold = resumes(ctx)
    with pytest.raises(NotSupportedException, match="resumed after an end block"):
        ctx.Render(np.zeros((2, B * 40), np.float32), B * 40, 0)
    del hold
    ctx.Dispose()


# ---- 7. buffers of more than one channel ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("nch,swap", [(2, 0), (3, 0), (2, 1), (3, 2)])   # swap: the Buffer replaced before Start by one of `swap` channels
def test_multichannel_buffer(nch, swap, form):
    def build(ctx):
        s = src(ctx, region_buffer(20, 9000, 0, 9000, nch=nch), 44100, ls=555, le=8000)
        if swap:
            s.Buffer = PlayableAudioBuffer.FromChannelArrays(region_buffer(21, 7000, 0, 7000, nch=swap), 22050)
        hold = _lfo(ctx, 5.0, 0.2, s.PlaybackRate)
        s.Connect(ctx.Destination)
        s.Start()
        return (s,) + hold
    ref, got = both(build, B * 80, form, ch=4 if nch == 3 and not swap else 2)
    # the edge: the output has the channels of the buffer that plays (a mono buffer is up-mixed: both channels the same)
    assert G.rms(ref[0]) > 1e-3 and (G.rms(ref[0] - ref[1]) > 1e-3) == (swap != 1)
    assert np.array_equal(ref, got)


def test_buffer_swap_while_resampling_refused():
    ctx = OfflineAudioContext(SR)
    ctx.Destination.SetChannelCount(2)
    s = src(ctx, region_buffer(22, 9000, 0, 9000, nch=2), 44100)
    hold = _lfo(ctx, 5.0, 0.2, s.PlaybackRate)
    s.Connect(ctx.Destination)
    s.Start()
    out = np.zeros((2, B * 40), np.float32)
    ctx.Render(out, B * 20, 0)
    assert G.rms(out[:, :B * 20]) > 1e-3
    s.Buffer = PlayableAudioBuffer.FromChannelArrays(region_buffer(23, 9000, 0, 9000, nch=3), 44100)
    with pytest.raises(NotSupportedException, match="resampler holds samples"):
        ctx.Render(out, B * 20, B * 20)
    del hold
    ctx.Dispose()


# ---- 8. the copy path at a non-unit buffer ratio ---------------------------------------------------------------------------------

def copy_path(ctx):
    """A 24 kHz buffer: the rate reaches exactly 2.0 on some blocks (effectiveRate == 1.0: the copy path, which leaves the
    resampler's window stale), resampling under an LFO in between."""
    s = src(ctx, [G.voice(24, 40000)], 24000, ls=300, le=39000)
    s.PlaybackRate.Value = 1.0
    g = _lfo(ctx, 6.0, 0.3, s.PlaybackRate, start=0.0, stop=B * 20 / SR)
    lfo2 = _lfo(ctx, 4.0, 0.25, s.PlaybackRate, start=B * 40 / SR, stop=B * 60 / SR)
    cs = timeline(ctx, s.PlaybackRate, [(B * 20 / SR, 1.0), (B * 40 / SR, 0.0), (B * 60 / SR, 1.0), (B * 70 / SR, 0.0)])
    s.Connect(ctx.Destination)
    s.Start()
    return (s, cs) + g + lfo2


def copied_blocks(out, buf):
    """Blocks of `out` that are a contiguous slice of `buf` (the copy path; a resampled block is not)."""
    where = {float(v): i for i, v in enumerate(buf)}
    res = []
    for b in range(out.shape[1] // B):
        blk = out[0, b * B:(b + 1) * B]
        i = where.get(float(blk[0]))
        if i is not None and blk[0] != 0 and i + B <= len(buf) and np.array_equal(blk, buf[i:i + B]):
            res.append(b)
    return res


@pytest.mark.parametrize("form", list(FORMS))
def test_copy_path_at_buffer_ratio_one_half(form):
    frames = B * 90
    ref, got = both(copy_path, frames, form, ch=1)
    # the edge: copied blocks in 20..39 and 60..69 only, resampled blocks before, between and after
    cp = copied_blocks(ref, G.voice(24, 40000))
    assert set(range(21, 39)) <= set(cp) and set(range(61, 69)) <= set(cp)
    assert not set(cp) & (set(range(0, 20)) | set(range(41, 60)) | set(range(71, 90)))
    assert G.rms(ref[:, B * 41:B * 59]) > 1e-3 and tail_sounds(ref)
    assert np.array_equal(ref, got)


# ---- 9. more than 64 modulated sources of different geometry in one chunk --------------------------------------------------------

def crowd(ctx):
    hold = []
    rng = np.random.default_rng(99)
    for v in range(80):
        sr = int(rng.choice([SR, 44100, 22050, 32000]))
        n = int(rng.integers(600, 9000))
        nch = int(rng.choice([1, 1, 2, 3]))
        loop = bool(rng.random() < 0.6)
        ls = int(rng.integers(0, n // 2))
        le = int(rng.choice([0, n + 100, int(rng.integers(ls + 1, n))]))
        s = src(ctx, region_buffer(200 + v, n, 0, n, nch=nch), sr, loop=loop, ls=ls if loop else None, le=le if loop else None)
        g = GainNode(ctx)
        g.Gain.Value = 0.1
        s.Connect(g).Connect(ctx.Destination)
        when = float(rng.choice([0.0, rng.uniform(0, 0.03)]))
        offset = float(rng.choice([0.0, rng.uniform(0, n / sr / 2)]))
        if rng.random() < 0.3:
            s.Start(when, offset, float(rng.uniform(0.01, 0.2)))
        else:
            s.Start(when, offset)
        if rng.random() < 0.2:
            s.Stop(float(rng.uniform(when, 0.25)))
        hold += [s, g, *_lfo(ctx, float(rng.uniform(1, 12)), float(rng.uniform(0.02, 0.5)), s.PlaybackRate)]
    return hold


@pytest.mark.parametrize("form", list(FORMS))
def test_80_sources_of_different_geometry(form):
    ref, got = both(crowd, B * 120, form)
    # the edge: sources end at different blocks (one-shots, durations, stops) while the loops keep sounding
    assert G.rms(ref[:, :B * 20]) > G.rms(ref[:, -B * 20:]) > 1e-3
    assert np.array_equal(ref, got)


# ---- the device walk against the host replay -------------------------------------------------------------------------------------

@pytest.mark.parametrize("case,frames", [(region_case(*r[1:]), FRAMES_REGION) for r in REGIONS[:3]] +
                                        [(fast_loop, B * 120)]
                         + [(short_case(n), B * 100) for n in SHORT]
                         + [(start_case(k), B * 90) for k in ["offset", "duration", "data_runs_out"]]
                         + [(crowd, B * 120)],
                         ids=[r[0] for r in REGIONS[:3]] + ["fast"] + [f"short{n}" for n in SHORT] + ["offset", "duration", "runs_out", "crowd"])
def test_walk_matches_host_replay(case, frames):
    walk_vs_host(case, frames)


def test_walk_matches_host_replay_end_then_audio():
    walk_vs_host(resumes, B * 40, chunk=1)


# ---- non-finite modulation: Math.Clamp keeps a NaN (AudioParam.cs:123-135) --------------------------------------------------------

NONFINITE = {40: np.nan, 300: np.inf, 301: -np.inf, 555: np.nan, 777: np.inf, 778: -np.inf}   # frames of a 1,000-frame loop


def nonfinite_source(ctx):
    x = G.voice(30, 1000, scale=0.3)
    for i, v in NONFINITE.items():
        x[i] = v
    s = AudioBufferSourceNode(ctx)
    s.Buffer = PlayableAudioBuffer.FromMonoArray(x, SR)
    s.Loop = True
    s.Start()
    return s


@pytest.mark.parametrize("target", ["gain", "gain_automated", "pan", "offset"])
def test_nonfinite_modulation(target):
    def build(ctx):
        m = nonfinite_source(ctx)
        carrier = OscillatorNode(ctx)
        carrier.Frequency.Value = 440.0
        carrier.Start()
        if target.startswith("gain"):
            n = GainNode(ctx)
            if target == "gain_automated":
                n.Gain.SetValueAtTime(0.5, 0.0)
                n.Gain.LinearRampToValueAtTime(1.5, 0.05)
            else:
                n.Gain.Value = 0.5
            m.Connect(n.Gain)
            carrier.Connect(n).Connect(ctx.Destination)
        elif target == "pan":
            n = StereoPannerNode(ctx)
            n.Pan.Value = 0.2
            m.Connect(n.Pan)
            carrier.Connect(n).Connect(ctx.Destination)
        else:
            n = ConstantSourceNode(ctx)
            n.Offset.Value = 0.25
            m.Connect(n.Offset)
            n.Connect(ctx.Destination)
            n.Start()
        return (m, carrier, n)
    frames = B * 40
    ref = render(OracleContext, build, 2, frames)
    got = render(OfflineAudioContext, build, 2, frames)
    # the edge: the NaN of the modulation reaches the output of the reference at the looped frames
    nan_frames = np.flatnonzero(np.isnan(ref).any(axis=0))
    assert all(f % 1000 in NONFINITE for f in nan_frames) and len(nan_frames) >= 2 * (frames // 1000)
    assert np.isfinite(ref[:, :40]).all()
    assert np.array_equal(np.isnan(ref), np.isnan(got)), (np.flatnonzero(np.isnan(got).any(axis=0))[:8], nan_frames[:8])
    if target == "pan":
        # a pan that changes every sample re-derives the gains every sample: (float)cos((double)x) on the device, the C library's
        # cosf in the reference (libm class) -- the finite samples within the 1e-5 contract, the NaNs in place
        fin = ~np.isnan(ref)
        assert G.rms(ref[fin] - got[fin]) <= 1e-5
    else:
        assert np.array_equal(ref, got, equal_nan=True)
