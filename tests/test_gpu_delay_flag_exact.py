"""Option `delay_flag_exact`: a DelayNode's output flag read from its samples.

The reference raises the flag of a DelayNode's output buffer at the first output sample that is `!= 0f` and never clears it
(DelayNode.cs:58-97).  By default the device path predicts the flag from the flags of the blocks that went into the ring, which can
come early: a buffer that starts with digital silence is flagged non-silent from its first block.  A BiQuadFilterNode behind the
delay, frozen by silence with its state kept (BiQuadFilterNode.cs:103-108), then wakes up in the wrong block.  With the option on the
delay is rendered ahead of the rest of the chunk and the block in which its samples raise the flag is read back (delay_onset_kernel).

Every scene renders 40 blocks or fewer, three ways: as one piece, in uneven pieces, and with `max_chunk_blocks` = 5 (onsets in a
chunk's first block, its last block, and in no block of a chunk).  The nodes are bit-exact kinds: the assertion is array_equal with
the CPU oracle.  Every case first asserts a control on the oracle alone: with the leading zeros replaced by 1e-30 -- what the
prediction takes them for -- the oracle's own output moves by at least 1e-3 RMS, so the case can detect a flag that rises early."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from graphaudio_amd import (AudioBufferSourceNode, BiQuadFilterNode, DelayNode, FilterType, GainNode, NotSupportedException,
                            OfflineAudioContext, OscillatorNode, OscillatorType, PlayableAudioBuffer)
from tests import _graphs as G
from tests._fuzz import build_random_graph
from tests._oracle import OracleContext
from tests.test_gpu_playback_rate_mod import vibrato

SR = 48000
BLOCKS = 40
FRAMES = 128 * BLOCKS
FLT_MIN = np.float32(1.17549435e-38)

# how a scene is rendered on the device: (pieces, max_chunk_blocks)
WAYS = {"one_piece": (None, None), "uneven": ([128 * 3 + 5, 128 * 7 - 1, 77, 128 * 11 + 64, 1, 128 * 6], None), "chunks_of_5": (None, 5)}


def _noise(seed, n):
    x = G.voice(seed, n)
    x[x == 0] = np.float32(0.125)   # (the first sample behind the leading zeros has to be the onset)
    return x


def delayed_buffers(kind, lead=0.0):
    """The channels of the 2560-frame one-shot that feeds the delay; `lead` replaces the exact zeros in front (the control: 1e-30)."""
    n = 2560
    lead = np.float32(lead)
    if kind.startswith("z"):   # z832, z831, z805, z960: Z leading zeros
        z = int(kind[1:])
        x = _noise(11, n)
        x[:z] = lead
        return [x]
    if kind in ("stereo", "stereo_late"):   # channel 0 stays zero 300 frames longer than channel 1
        a, b = _noise(12, n), _noise(13, n)
        a[:805 + 300] = lead
        b[:805] = lead
        return [a, b]
    if kind == "negzero":   # leading -0.0f: `!= 0f` is false for them
        x = _noise(14, n)
        x[:805] = lead if lead != 0 else np.float32(-0.0)
        return [x]
    if kind == "fltmin":   # behind leading -0.0f one FLT_MIN sample, 700 zeros, then noise: that sample raises the flag
        x = _noise(15, n)
        x[:300] = lead if lead != 0 else np.float32(-0.0)
        x[300] = FLT_MIN
        x[301:1001] = lead
        return [x]
    if kind == "denormal":   # one subnormal sample (1e-40), 700 zeros, then noise: `!= 0f` holds for it, a flushed compare would miss it
        x = _noise(16, n)
        x[:300] = lead
        x[300] = np.float32(1e-40)
        x[301:1001] = lead
        return [x]
    raise ValueError(kind)


def base_scene(ctx, kind, lead=0.0, chorus=False):
    """A 384-frame burst into a low-pass biquad (200 Hz, Q 8) whose second connection is DelayNode(0.05) at 0.02 s, fed by a one-shot
    that starts with digital silence.  The biquad keeps its state while both are silent and rings on when the delay's flag rises."""
    burst = AudioBufferSourceNode(ctx)
    burst.Buffer = PlayableAudioBuffer.FromMonoArray(_noise(3, 384), SR)
    bq = BiQuadFilterNode(ctx)
    bq.Type = FilterType.Lowpass
    bq.Frequency.Value = 200.0
    bq.Q.Value = 8.0
    late = AudioBufferSourceNode(ctx)
    late.Buffer = PlayableAudioBuffer.FromChannelArrays(delayed_buffers(kind, lead), SR)
    d = DelayNode(ctx, 0.05)
    d.DelayTime.Value = 0.02
    hold = [burst, bq, late, d]
    if chorus:   # a 2 Hz triangle (the sine differs from the C library's in the last bit now and then, and the delay time is quantised)
        lfo = OscillatorNode(ctx)
        lfo.Type = OscillatorType.Triangle
        lfo.Frequency.Value = 2.0
        depth = GainNode(ctx)
        depth.Gain.Value = 0.005
        lfo.Connect(depth)
        depth.Connect(d.DelayTime)
        lfo.Start()
        hold += [lfo, depth]
    burst.Connect(bq)
    late.Connect(d)
    d.Connect(bq)
    bq.Connect(ctx.Destination)
    burst.Start()
    # stereo_late: the one-shot starts inside block 1 -- the delay's buffer is re-rented (1 -> 2 channels, DelayNode.cs:50-56) inside a
    # chunk, and the biquad sizes its input from the delay's channel count of the block before (AudioNodeInput.cs:140-168)
    late.Start(0.004 if kind == "stereo_late" else 0.0)
    return hold


def two_delays(ctx, kind, lead=0.0):
    """D1 -> biquad -> D2 -> destination: D1's flag is read, D2 (an undecided delay in front of it) keeps the prediction; nothing behind
    D2 reads its flag."""
    hold = base_scene(ctx, kind, lead)
    bq = hold[1]
    bq.Disconnect(ctx.Destination)
    d2 = DelayNode(ctx, 0.05)
    d2.DelayTime.Value = 0.01
    bq.Connect(d2)
    d2.Connect(ctx.Destination)
    return hold + [d2]


def with_vibrato(ctx, kind, lead=0.0):
    """The base scene next to a voice whose playbackRate is modulated: both kinds of stage-1 work in one chunk."""
    return list(vibrato(ctx)) + base_scene(ctx, kind, lead)


def render(mk, build, frames=FRAMES, pieces=None, opts=None, ch=1):
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
    stats = ctx.GetStats() if mk is OfflineAudioContext else None
    del hold
    ctx.Dispose()
    return out, stats


SCENES = {"base": base_scene, "chorus": functools.partial(base_scene, chorus=True), "two_delays": two_delays, "vibrato": with_vibrato}


@functools.lru_cache(maxsize=None)
def oracle(scene, kind, lead=0.0):
    out, _ = render(OracleContext, lambda ctx: SCENES[scene](ctx, kind, lead))
    out.setflags(write=False)
    return out


def control(scene, kind):
    """The case can detect an early flag: a condition on the oracle alone, not a tolerance."""
    moved = G.rms(oracle(scene, kind) - oracle(scene, kind, 1e-30))
    assert moved >= 1e-3, (scene, kind, moved)


def device(scene, kind, way, on=True):
    pieces, chunk = WAYS[way]
    opts = {"delay_flag_exact": 1 if on else 0}
    if chunk:
        opts["max_chunk_blocks"] = chunk
    return render(OfflineAudioContext, lambda ctx: SCENES[scene](ctx, kind), pieces=pieces, opts=opts)


@pytest.mark.parametrize("way", list(WAYS))
# (z960: frame 0 of block 15, the first block of a chunk of 5; z832: the last block of one; fltmin: block 9, the last block of one)
@pytest.mark.parametrize("kind", ["z832", "z831", "z805", "stereo", "negzero", "fltmin", "z960", "stereo_late", "denormal"])
def test_base_scene(kind, way):
    control("base", kind)
    got, st = device("base", kind, way)
    assert np.array_equal(oracle("base", kind), got)
    assert st["delay_flags_read"] > 0


@pytest.mark.parametrize("way", list(WAYS))
def test_chorus_scene(way):
    control("chorus", "z805")
    got, st = device("chorus", "z805", way)
    assert np.array_equal(oracle("chorus", "z805"), got)
    assert st["delay_flags_read"] > 0


@pytest.mark.parametrize("way", list(WAYS))
def test_two_delays_in_a_row(way):
    control("two_delays", "z805")
    got, st = device("two_delays", "z805", way)
    assert np.array_equal(oracle("two_delays", "z805"), got)
    assert st["delay_flags_read"] > 0 and st["delay_flags_predicted"] > 0


@pytest.mark.parametrize("way", list(WAYS))
def test_with_a_vibrato_voice(way):
    control("vibrato", "z805")
    got, st = device("vibrato", "z805", way)
    assert np.array_equal(oracle("vibrato", "z805"), got)
    assert st["delay_flags_read"] > 0


# ---- delays the option leaves to the prediction ------------------------------------------------------------------------------

def delay_on_a_loop(ctx):
    """gain -> biquad -> delay -> gain -> back to the first gain, excited by one block."""
    s = AudioBufferSourceNode(ctx)
    s.Buffer = PlayableAudioBuffer.FromMonoArray(_noise(21, 256), SR)   # (the block in which a one-shot runs out is cleared: one block of audio)
    g1, g2 = GainNode(ctx), GainNode(ctx)
    g2.Gain.Value = 0.5
    bq = BiQuadFilterNode(ctx)
    bq.Frequency.Value = 1500.0
    d = DelayNode(ctx, 0.05)
    d.DelayTime.Value = 0.01
    s.Connect(g1)
    g1.Connect(bq)
    bq.Connect(d)
    d.Connect(g2)
    g2.Connect(g1)
    g1.Connect(ctx.Destination)
    s.Start()
    return [s, g1, g2, bq, d]


def delay_on_a_loop_closed_through_a_finished_node(ctx):
    """src -> X -> destination, X -> Y -> X, Y -> W(delay) -> X, with X's connections in the order Y, W: the reference's walk closes
    the loop X -> Y -> X first and finishes Y before it reaches W, so W is on no back edge's stack -- but X and Y, which W's cone
    holds, consume W."""
    s = AudioBufferSourceNode(ctx)
    s.Buffer = PlayableAudioBuffer.FromMonoArray(_noise(22, 256), SR)
    x, y = GainNode(ctx), GainNode(ctx)
    y.Gain.Value = 0.4
    w = DelayNode(ctx, 0.05)
    w.DelayTime.Value = 0.01
    x.Connect(y)
    y.Connect(x)
    y.Connect(w)
    w.Connect(x)
    s.Connect(x)
    x.Connect(ctx.Destination)
    s.Start()
    return [s, x, y, w]


def delay_behind_a_modulated_rate(ctx):
    hold = vibrato(ctx)
    s = hold[0]
    s.Disconnect(ctx.Destination)
    d = DelayNode(ctx, 0.05)
    d.DelayTime.Value = 0.01
    s.Connect(d)
    d.Connect(ctx.Destination)
    return list(hold) + [d]


@pytest.mark.parametrize("way", list(WAYS))
@pytest.mark.parametrize("build", [delay_on_a_loop, delay_on_a_loop_closed_through_a_finished_node, delay_behind_a_modulated_rate])
def test_fallback_keeps_the_prediction(build, way):
    pieces, chunk = WAYS[way]
    outs = []
    for on in (1, 0):
        opts = {"delay_flag_exact": on}
        if chunk:
            opts["max_chunk_blocks"] = chunk
        out, st = render(OfflineAudioContext, build, pieces=pieces, opts=opts)
        outs.append(out)
        if on:
            assert st["delay_flags_read"] == 0 and st["delay_flags_predicted"] > 0
    assert G.rms(outs[0]) > 1e-4
    assert np.array_equal(outs[0], outs[1])


def test_idle_delay_reads_nothing():
    """A DelayNode nothing feeds, next to a playing voice: accepted chunk after chunk, never probed."""
    def build(ctx):
        s = AudioBufferSourceNode(ctx)
        s.Buffer = PlayableAudioBuffer.FromMonoArray(_noise(31, FRAMES), SR)
        d = DelayNode(ctx, 0.05)
        s.Connect(ctx.Destination)
        d.Connect(ctx.Destination)
        s.Start()
        return [s, d]
    ref, _ = render(OracleContext, build)
    got, st = render(OfflineAudioContext, build, opts={"delay_flag_exact": 1, "max_chunk_blocks": 5})
    assert np.array_equal(ref, got)
    assert st["delay_flags_read"] == 0


# ---- no regression where the prediction was right: generated graphs, the bounds of test_gpu_fuzz.test_random_graph_matches_oracle ----

@pytest.mark.parametrize("seed", list(range(40)) + [20256, 22316] + list(range(50000, 50008)))
def test_random_graph_with_the_option_on(seed):
    frames = 128 * 36
    o = OracleContext(48000)
    ch = build_random_graph(o, seed, frames)
    ref = np.zeros((ch, frames), np.float32)
    try:
        o.Render(ref, frames)
    except Exception as e:  # e.g. destination narrower than requested: must fail the same way on the device
        h = OfflineAudioContext(48000)
        h.SetOption("delay_flag_exact", 1)
        build_random_graph(h, seed, frames)
        with pytest.raises(type(e)):
            h.Render(np.zeros((ch, frames), np.float32), frames)
        return

    def device(on):
        h = OfflineAudioContext(48000)
        h.SetOption("max_chunk_blocks", 11)
        h.SetOption("coarse_min_blocks", 1 << 30)
        h.SetOption("delay_flag_exact", on)
        build_random_graph(h, seed, frames)
        got = np.zeros_like(ref)
        pos = 0
        rng = np.random.default_rng(1000 + seed)
        while pos < frames:
            n = int(min(frames - pos, rng.integers(1, 128 * 9)))
            h.Render(got, n, pos)
            pos += n
        return h, got, pos

    try:
        h, got, pos = device(1)
    except NotSupportedException as e:
        with pytest.raises(NotSupportedException):   # the option refuses nothing of its own: the graph is refused without it too
            device(0)
        pytest.skip(f"graph uses a feature outside the device path: {e}")
    assert o.CurrentBlock == h.CurrentBlock or pos == frames
    if seed >= 50000 and (not np.isfinite(ref).all() or G.rms(ref) > 50.0):
        pytest.skip("a feedback loop with a gain above 1: the reference's output is not finite, or grows without bound and every last-bit difference with it")
    err = G.rms(ref - got)
    scale = max(G.rms(ref), 1e-3)
    assert err <= 1e-5 * max(1.0, scale if seed >= 50000 else 1.0) and err <= 2e-5 * scale, (seed, err, scale)
