"""Impulse responses of 131,073 .. 1,048,576 taps on formulation D: the partition sum in segments of 16 coarse partitions
(graphaudio_amd/csrc/ga_coarse.hip, coarse_sum_seg_kernel / coarse_mac_seg_kernel; option coarse_long).

Bounds.  TOL_RMS = 1e-5 absolute and REL = 2e-6 are the bounds of tests/test_gpu_coarse.py.  The oracle's own float32 partition
sum drifts from float64 about as sqrt(P) (tests/test_oracle_long_ir.py pins it: 1.1e-6 at 262,144 taps, 1.55e-6 at 524,288), so
every case measures the oracle against the float64 model of the same case (`o64`, relative RMS) and asks
    device vs float64 model : relative RMS <= max(REL, o64)
    device vs oracle        : RMS <= TOL_RMS  and  relative RMS <= REL + o64.
The float64 models are linear convolutions written from the definition (tests/_f64model.py); where a case edits the graph
between renders the model applies the reference's rules (a new voice starts at the current frame; a disposed convolver is
silent from then on; a new impulse response starts from an empty delay line, ConvolverNode.cs:51-77).  `o64 <= 1e-5` is
asserted first: a model that does not describe the case would otherwise widen the bound.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from graphaudio_amd import AudioBufferSourceNode, ConvolverNode, OfflineAudioContext, PlayableAudioBuffer
from tests import _f64model as M
from tests import _graphs as G
from tests._oracle import OracleContext

SR = 48000
TOL_RMS = 1e-5
REL = 2e-6
_oracle_cache = {}


def hip(**opts):
    ctx = OfflineAudioContext(SR)
    ctx.SetOption("coarse_min_blocks", 1)
    for k, v in opts.items():
        ctx.SetOption(k, v)
    return ctx


def used_coarse(st):
    return st["stage_launches"][5] > 0 and st["stage_launches"][3] == 0   # coarse_fwd ran, no A/B/C partition sum


def blocks_for(taps):
    """whole blocks, every partition populated: frames >= taps + 128 * 64"""
    return (taps + 128 * 64 + 127) // 128


def oracle(key, builder, frames):
    if key not in _oracle_cache:
        o = OracleContext(SR)
        ch = builder(o)
        _oracle_cache[key] = G.render(o, ch, frames)
        o.Dispose()
    return _oracle_cache[key]


def render_hip(builder, frames, channels, pieces=None, **opts):
    h = hip(**opts)
    builder(h)
    got = np.zeros((channels, frames), np.float32)
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
    return got, st


def bounds(name, ref, got, model, part=slice(None)):
    """the three figures of a case (printed: DESIGN.md section 2a holds the table) and the two assertions"""
    ref, got, model = ref[:, part], got[:, part], model[:, part]
    sig = M.rms(model)
    assert sig > 1e-5
    o64 = M.rms(ref - model) / sig
    d64 = M.rms(got - model) / sig
    dor = M.rms(got - ref)
    print(f"LONGIR {name}: oracle-vs-f64 {o64:.3e}  device-vs-f64 {d64:.3e}  device-vs-oracle {dor:.3e} abs {dor / M.rms(ref):.3e} rel")
    assert o64 <= 1e-5, ("the float64 model does not describe the case", o64)
    assert d64 <= max(REL, o64), (d64, o64)
    assert dor <= TOL_RMS, dor
    assert dor <= (REL + o64) * M.rms(ref), (dor / M.rms(ref), o64)


# ---- 1. tap counts: P' = 17 (one partition in the second segment, one tap in it), 17 whole, 25, 32, 64 ------------------------
@pytest.mark.parametrize("taps", [131073, 139264, 200000, 262144, 524288])
def test_tap_counts(taps):
    frames = 128 * blocks_for(taps)
    build = lambda c: G.config3_convolver(c, voices=3, taps=taps, frames=frames)
    got, st = render_hip(build, frames, 2)
    assert used_coarse(st), st["stage_launches"]
    ref = oracle(("cfg3", 3, taps, frames), build, frames)
    model = M.config3_shared(3, taps, frames)
    bounds(f"shared x3 {taps}", ref, got, model)
    bounds(f"shared x3 {taps} steady", ref, got, model, slice(taps, None))


# ---- 2. the longest response: P' = 128, eight segments ---------------------------------------------------------------------
def test_1048576_taps_one_voice_one_channel():
    """(the oracle takes about a minute on one core here)"""
    taps = 1048576
    frames = 128 * blocks_for(taps)
    build = lambda c: G.config3_convolver(c, voices=1, taps=taps, frames=frames, ir_channels=1)
    got, st = render_hip(build, frames, 1)
    assert used_coarse(st), st["stage_launches"]
    ref = oracle(("cfg3-1ch", 1, taps, frames), build, frames)
    model = M.config3_shared(1, taps, frames, ir_channels=1)
    bounds(f"one voice {taps}", ref, got, model)
    bounds(f"one voice {taps} steady", ref, got, model, slice(taps, None))


# ---- 3. routes, each at 200,000 taps (P' = 25: a whole segment and one of 9 -> 12 partitions) ----------------------------------
RT = 200000
RF = 128 * blocks_for(RT)


def test_route_private_response_per_voice():
    """impulse responses of their own: the general kernel, terms expanded into (signal, segment) pairs"""
    build = lambda c: G.config3_convolver(c, voices=5, taps=RT, frames=RF, shared=False)
    got, st = render_hip(build, RF, 2)
    assert used_coarse(st) and "coarse_mac_seg_kernel" in " ".join(st["stage_kernel"]), st["stage_kernel"]
    bounds("private x5", oracle(("cfg3p", 5, RT, RF), build, RF), got, M.config3_private(5, RT, RF))


def _true_stereo(ctx):
    s = AudioBufferSourceNode(ctx)
    s.Buffer = PlayableAudioBuffer.FromStereoArrays(G.voice(50, RF + 256), G.voice(51, RF + 256), SR)
    cv = ConvolverNode(ctx)
    cv.Buffer = PlayableAudioBuffer.FromChannelArrays([G.synth_ir(c, RT) for c in range(4)], SR)
    s.Connect(cv).Connect(ctx.Destination)
    s.Start()
    return 2


def test_route_true_stereo_four_channels():
    """outL = L * h0 + R * h2, outR = L * h1 + R * h3 (ConvolverNode.cs:127-151)"""
    got, st = render_hip(_true_stereo, RF, 2)
    assert used_coarse(st)
    x = [G.voice(50, RF + 256)[:RF].astype(np.float64), G.voice(51, RF + 256)[:RF].astype(np.float64)]
    h = [M.scaled_ir64(G.synth_ir(c, RT)) for c in range(4)]
    model = np.stack([M.linear_conv(x[0], h[0], RF) + M.linear_conv(x[1], h[2], RF), M.linear_conv(x[0], h[1], RF) + M.linear_conv(x[1], h[3], RF)])
    bounds("true stereo", oracle("true-stereo", _true_stereo, RF), got, model)


def _stereo_discrete(ctx):
    s = AudioBufferSourceNode(ctx)
    s.Buffer = PlayableAudioBuffer.FromStereoArrays(G.voice(60, RF + 256), G.voice(61, RF + 256), SR)
    cv = ConvolverNode(ctx)
    cv.EnableTrueStereo = False
    cv.Buffer = PlayableAudioBuffer.FromChannelArrays([G.synth_ir(c, RT) for c in range(2)], SR)
    s.Connect(cv).Connect(ctx.Destination)
    s.Start()
    return 2


def test_route_stereo_discrete():
    got, st = render_hip(_stereo_discrete, RF, 2)
    assert used_coarse(st)
    model = np.stack([M.linear_conv(G.voice(60 + c, RF + 256)[:RF].astype(np.float64), M.scaled_ir64(G.synth_ir(c, RT)), RF) for c in range(2)])
    bounds("stereo discrete", oracle("stereo-discrete", _stereo_discrete, RF), got, model)


def test_route_sixteen_channel_response():
    """16 columns of one signal: four 4-column pieces (16-column pieces are made for P' <= 4 only)"""
    build = lambda c: G.config5_ambisonic(c, sources=1, taps=RT, frames=RF)
    got, st = render_hip(build, RF, 16)
    assert used_coarse(st)
    bounds("16 channels", oracle("cfg5", build, RF), got, M.config5(1, RT, RF))


@pytest.mark.parametrize("opt", ["coarse_premix", "coarse_tail"])
def test_route_without_premix_or_tail(opt):
    """coarse_premix = 0: the members' spectra are summed per segment (coarse_sum_seg_kernel with three terms);
    coarse_tail = 0: input histories only, in two chunks so that the second starts from them"""
    build = lambda c: G.config3_convolver(c, voices=3, taps=RT, frames=RF)
    got, st = render_hip(build, RF, 2, pieces=[128 * 900], **{opt: 0})
    assert used_coarse(st)
    if opt == "coarse_tail":
        assert st["coarse_carried_outputs"] == 0
    bounds(f"{opt}=0", oracle(("cfg3", 3, RT, RF), build, RF), got, M.config3_shared(3, RT, RF))


# ---- 4. state ---------------------------------------------------------------------------------------------------------------
ST = 300000


def test_state_uneven_pieces_equal_one_call():
    """one-block chunks, chunks far shorter than the 37-partition history (several in a row), max_chunk_blocks = 96, partial blocks"""
    frames = 128 * 2500 + 60
    build = lambda c: G.config3_convolver(c, voices=3, taps=ST, frames=frames)
    pieces = [100, 128 * 3 + 7, 1, 128 * 70, 128, 128, 128 * 700 - 5, 128 * 40, 128 * 40, 77, 128 * 1000]
    one, st1 = render_hip(build, frames, 2, max_chunk_blocks=32768)
    got, st = render_hip(build, frames, 2, pieces=pieces, max_chunk_blocks=96)
    assert used_coarse(st1) and used_coarse(st) and st["chunks"] > 25
    ref = oracle(("cfg3", 3, ST, frames), build, frames)
    model = M.config3_shared(3, ST, frames)
    bounds("one call 300000", ref, one, model)
    bounds("uneven pieces 300000", ref, got, model)
    # the two renders round differently (carried tails against histories): both sit inside the bound around the float64 model
    o64 = M.rms(ref - model) / M.rms(model)
    assert M.rms(got - one) <= 2 * max(REL, o64) * M.rms(model)


def test_state_group_edit_between_renders():
    """a voice joins, a voice is disposed: each time the tail of the old group is dropped and the members' histories (37 coarse
    blocks each, longer than the chunks) take over"""
    taps = ST
    steps = [128 * 1100, 128 * 300, 128 * 700, 128 * 200, 128 * 500]
    total = sum(steps)

    def run(ctx):
        shared = PlayableAudioBuffer.FromChannelArrays([G.synth_ir(c, taps) for c in range(2)], SR)
        ctx.Destination.SetChannelCount(2)
        voices = []

        def add(v):
            s = AudioBufferSourceNode(ctx)
            s.Buffer = PlayableAudioBuffer.FromMonoArray(G.voice(v, total + 256), SR)
            cv = ConvolverNode(ctx)
            cv.Buffer = shared
            s.Connect(cv).Connect(ctx.Destination)
            s.Start()
            voices.append((s, cv))
        out = np.zeros((2, total), np.float32)
        pos = 0
        for v in range(3):
            add(v)
        for i, n in enumerate(steps):
            if i == 2:
                add(3)                     # joins at steps[0] + steps[1]
            if i == 3:
                voices[0][1].Dispose()     # silent from steps[0] + steps[1] + steps[2] on
            ctx.Render(out, n, pos)
            pos += n
        return out

    o = OracleContext(SR)
    ref = run(o)
    o.Dispose()
    h = hip()
    got = run(h)
    st = h.GetStats()
    h.Dispose()
    assert used_coarse(st) and st["coarse_carried_outputs"] >= 2
    join, gone = steps[0] + steps[1], steps[0] + steps[1] + steps[2]
    hs = [M.scaled_ir64(G.synth_ir(c, taps)) for c in range(2)]
    model = np.zeros((2, total))
    for v in range(4):
        x = np.zeros(total)
        start = join if v == 3 else 0
        x[start:] = G.voice(v, total + 256)[:total - start]
        for c in range(2):
            y = M.linear_conv(x, hs[c], total)
            if v == 0:
                y[gone:] = 0.0
            model[c] += y
    bounds("group edit", ref, got, model)


def test_state_impulse_response_swap_on_a_live_node():
    """131,072 -> 300,000 -> 20,000 taps: one sweep, the segmented sum, one sweep; every swap starts from an empty delay line"""
    steps = [(131072, 128 * 1200), (300000, 128 * 2500), (20000, 128 * 400)]
    total = sum(n for _, n in steps)

    def run(ctx):
        s = AudioBufferSourceNode(ctx)
        s.Buffer = PlayableAudioBuffer.FromMonoArray(G.voice(7, total + 256), SR)
        cv = ConvolverNode(ctx)
        s.Connect(cv).Connect(ctx.Destination)
        s.Start()
        out = np.zeros((2, total), np.float32)
        pos = 0
        for i, (taps, n) in enumerate(steps):
            cv.Buffer = PlayableAudioBuffer.FromChannelArrays([G.synth_ir(c, taps, seed0=7 + 30 * i) for c in range(2)], SR)
            ctx.Render(out, n, pos)
            pos += n
        return out

    o = OracleContext(SR)
    ref = run(o)
    o.Dispose()
    h = hip()
    got = run(h)
    st = h.GetStats()
    h.Dispose()
    assert used_coarse(st)
    x = G.voice(7, total + 256)[:total].astype(np.float64)
    model = np.zeros((2, total))
    pos = 0
    for i, (taps, n) in enumerate(steps):
        for c in range(2):
            model[c, pos:pos + n] = M.linear_conv(x[pos:], M.scaled_ir64(G.synth_ir(c, taps, seed0=7 + 30 * i)), n)
        pos += n
    bounds("response swap", ref, got, model)


def test_state_exact_zeros_in_front_of_a_late_source():
    """the response to nothing is the zero page: a source that starts in block 700 of a render in chunks of 96 blocks"""
    taps, onset = RT, 700
    frames = 128 * 1800

    def build(ctx):
        s = AudioBufferSourceNode(ctx)
        s.Buffer = PlayableAudioBuffer.FromMonoArray(G.voice(11, frames), SR)
        cv = ConvolverNode(ctx)
        cv.Buffer = PlayableAudioBuffer.FromChannelArrays([G.synth_ir(c, taps) for c in range(2)], SR)
        s.Connect(cv).Connect(ctx.Destination)
        s.Start(onset * 128 / SR + 1e-4)   # (block-granular start: the first block whose end lies behind this time)
        return 2

    ref = oracle("late-source", build, frames)
    first = int(np.flatnonzero(np.any(ref != 0, axis=0))[0])
    assert first >= onset * 128
    for opts in ({"max_chunk_blocks": 96}, {}):
        got, st = render_hip(build, frames, 2, **opts)
        assert used_coarse(st)
        assert not np.any(got[:, :first]), (opts, int(np.flatnonzero(np.any(got != 0, axis=0))[0]), first)
        x = np.zeros(frames)
        x[first:] = G.voice(11, frames)[:frames - first]
        model = np.stack([M.linear_conv(x, M.scaled_ir64(G.synth_ir(c, taps)), frames) for c in range(2)])
        bounds(f"late source {opts}", ref, got, model)


def test_state_private_responses_in_short_pieces_with_a_silent_stretch():
    """the general kernel's (signal, segment) pairs with histories in front (u_lo = -(P' - 1)), chunks of <= 96 blocks against a
    25-partition history for many chunks in a row, job ranges with t0 > 0 in the long piece; the first convolver's source ends
    after 500 blocks and a second source on the SAME convolver starts in block 1500: sound after a silent stretch"""
    taps, onset = RT, 1500
    frames = 128 * 2700 + 40

    def irs(v):
        return [G.synth_ir(c, taps, seed0=7 + 100 * (v + 1)) for c in range(2)]

    def build(ctx):
        ctx.Destination.SetChannelCount(2)
        for v in range(3):
            s = AudioBufferSourceNode(ctx)
            s.Buffer = PlayableAudioBuffer.FromMonoArray(G.voice(v, 128 * 500 if v == 0 else frames + 256), SR)
            cv = ConvolverNode(ctx)
            cv.Buffer = PlayableAudioBuffer.FromChannelArrays(irs(v), SR)
            s.Connect(cv).Connect(ctx.Destination)
            s.Start()
            if v == 0:
                late = AudioBufferSourceNode(ctx)
                late.Buffer = PlayableAudioBuffer.FromMonoArray(G.voice(20, frames), SR)
                late.Connect(cv)
                late.Start(onset * 128 / SR + 1e-4)   # (block-granular start: block `onset`)
        return 2

    pieces = [128 * 90, 100, 128 * 3 + 7, 1, 128 * 40, 128 * 40, 128 * 40, 128 * 700 - 5, 128, 77, 128 * 30, 128 * 30]
    got, st = render_hip(build, frames, 2, pieces=pieces, max_chunk_blocks=96)
    assert used_coarse(st) and st["chunks"] > 25 and "coarse_mac_seg_kernel" in " ".join(st["stage_kernel"]), st["stage_kernel"]
    one, st1 = render_hip(build, frames, 2, max_chunk_blocks=32768)   # (one chunk: jobs at t0 = 0 and t0 = 32 or 72)
    assert used_coarse(st1) and st1["chunks"] == 1
    model = np.zeros((2, frames))
    for v in range(3):
        x = np.zeros(frames)
        if v == 0:
            x[:128 * 499] = G.voice(0, 128 * 500)[:128 * 499]   # (the reference's source ends with the last block that is followed by more samples)
            x[onset * 128:] += G.voice(20, frames)[:frames - onset * 128]
        else:
            x[:] = G.voice(v, frames + 256)[:frames]
        for c in range(2):
            model[c] += M.linear_conv(x, M.scaled_ir64(irs(v)[c]), frames)
    ref = oracle("private-pieces", build, frames)
    bounds("private x3 short pieces, silent stretch", ref, got, model)
    bounds("private x3 one chunk, silent stretch", ref, one, model)


def test_long_group_beside_unfused_short_responses_at_one_depth():
    """Every Y row of a stage is as long as the stage's longest carried tail: two voices that share a 288,000-tap response (pre-mixed,
    tail of 37 blocks) stretch the rows of twelve unfused stereo convolvers of 65,536 taps at the same depth (each feeds a gain of
    its own).  The Y arena has to be sized for that."""
    frames = 128 * 1000
    gains = [0.5 + 0.03 * v for v in range(12)]

    def build(ctx):
        from graphaudio_amd import GainNode
        ctx.Destination.SetChannelCount(2)
        long_ir = PlayableAudioBuffer.FromChannelArrays([G.synth_ir(c, 288000) for c in range(2)], SR)
        for v in range(14):
            s = AudioBufferSourceNode(ctx)
            s.Buffer = PlayableAudioBuffer.FromMonoArray(G.voice(v, frames + 256), SR)
            cv = ConvolverNode(ctx)
            s.Connect(cv)
            if v < 2:
                cv.Buffer = long_ir
                cv.Connect(ctx.Destination)
            else:
                cv.Buffer = PlayableAudioBuffer.FromChannelArrays([G.synth_ir(c, 65536, seed0=7 + 100 * v) for c in range(2)], SR)
                g = GainNode(ctx)
                g.Gain.Value = gains[v - 2]
                cv.Connect(g)
                g.Connect(ctx.Destination)
            s.Start()
        return 2

    model = np.zeros((2, frames))
    for v in range(14):
        x = G.voice(v, frames + 256)[:frames].astype(np.float64)
        for c in range(2):
            h = M.scaled_ir64(G.synth_ir(c, 288000)) if v < 2 else M.scaled_ir64(G.synth_ir(c, 65536, seed0=7 + 100 * v)) * float(np.float32(gains[v - 2]))
            model[c] += M.linear_conv(x, h, frames)
    ref = oracle("mixed-depth", build, frames)
    for pieces in (None, [128 * 300, 128 * 500]):
        got, st = render_hip(build, frames, 2, pieces=pieces)
        assert used_coarse(st)
        bounds(f"long group beside short unfused, pieces {pieces}", ref, got, model)


# ---- 5. A/B: coarse_long = 0 is the parent's plan (formulations A / B) --------------------------------------------------------
def test_coarse_long_switch():
    taps = 139264
    frames = 128 * blocks_for(taps)
    build = lambda c: G.config3_convolver(c, voices=3, taps=taps, frames=frames)
    ref = oracle(("cfg3", 3, taps, frames), build, frames)
    model = M.config3_shared(3, taps, frames)
    for on in (0, 1):
        got, st = render_hip(build, frames, 2, coarse_long=on)
        assert used_coarse(st) == (on == 1), (on, st["stage_launches"])
        bounds(f"coarse_long={on}", ref, got, model)


# ---- 6. beyond the limit: formulations A / B as before ------------------------------------------------------------------------
def test_1048577_taps_stay_on_the_direct_formulations():
    taps = 1048577
    frames = 128 * 24
    build = lambda c: G.config3_convolver(c, voices=1, taps=taps, frames=frames, ir_channels=1)
    got, st = render_hip(build, frames, 1)
    assert not used_coarse(st) and st["stage_launches"][3] > 0 and st["stage_launches"][5] == 0
    ref = oracle(("cfg3-1ch", 1, taps, frames), build, frames)
    bounds("1048577 taps", ref, got, M.config3_shared(1, taps, frames, ir_channels=1))
