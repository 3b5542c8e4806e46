"""Scenes of one to four nodes rendered as ONE chunk of production length, shared by tests/test_oracle_long_chunks.py (CPU: the
numpy models against the oracle, the two oracles against each other) and tests/test_gpu_long_chunks.py (the device against them).

Two lengths.  L1 = 2200 blocks with the default options: 34 full groups of 64 blocks and a ragged one of 24, past the grids capped
at 1024 and at 2048 blocks.  L2 = 4200 blocks with `max_chunk_blocks` = 8192: past the grids capped at 4096 blocks (524,288 frames).
Every scene's docstring names the kernel (ga_kernels.hip, ga_biquad.hip) and the boundary it crosses.  A scene is a _param_scenes.Scene: it is built
on any context (HIP product, oracle, double-trig oracle)."""
import functools
import math

import numpy as np

from graphaudio_amd import (AudioBufferSourceNode, AudioStreamSourceNode, BiQuadFilterNode, ChannelCountMode, ChannelMergerNode,
                            ConstantSourceNode, DelayNode, FilterType, GainNode, OfflineAudioContext, OscillatorNode, OscillatorType,
                            PlayableAudioBuffer)
from tests import _graphs as G
from tests import _param_scenes as P
from tests._oracle import DtrigOracleContext, OracleContext
from tests._param_scenes import B, F32, NYQ, SR, Scene, Timeline, at_frame, noise

L1 = 2200
L2 = 4200
L2_OPTS = {"max_chunk_blocks": 8192}
T = B / SR
GROUP = 64   # blocks per group of oscillator_kernel / stereo_panner_dynamic_kernel, per workgroup of resample_kernel / gsr_kernel / stream_kernel


# ---- rendering ---------------------------------------------------------------------------------------------------------------

def render(mk, scene, opts=None, pieces=None, chunks=None, probe=None):
    """(output, stats).  On the device every render call has to be ONE chunk (`chunks`: another expectation, for a render that is
    chunked on purpose): a chunk split silently by Context::chunkLimit would leave the boundary a scene targets uncrossed.
    `probe`: fn(what the scene's builder returned), called behind the last render call; its result is returned as a third value."""
    ctx = mk(SR)
    device = mk is OfflineAudioContext
    if device:
        for k, v in (opts or {}).items():
            ctx.SetOption(k, v)
    ctx.Destination.SetChannelCount(scene.ch)
    if scene.ch == 1:
        ctx.Destination.Inputs[0].SetChannelCount(1)
    hold = scene.build(ctx)
    out = np.zeros((scene.ch, scene.frames), F32)
    pos, calls = 0, 0
    for n in (pieces or [scene.frames]):
        ctx.Render(out, n, pos)
        pos, calls = pos + n, calls + 1
    assert pos == scene.frames
    st = ctx.GetStats() if device else None
    if device:
        assert st["chunks"] == (calls if chunks is None else chunks), (scene.name, st["chunks"], calls, chunks)
    seen = probe(hold) if probe else None
    del hold
    ctx.Dispose()
    return (out, st, seen) if probe else (out, st)


@functools.lru_cache(maxsize=None)
def _reference(mk, name):
    out, _ = render(mk, SCENES[name])
    out.setflags(write=False)
    return out


def oracle(name):
    """The plain oracle's render of SCENES[name]: computed once, shared, read-only."""
    return _reference(OracleContext, name)


def dtrig(name):
    return _reference(DtrigOracleContext, name)


def same(ref, got, what):
    """np.array_equal with the place of the first difference: frame, block, group of 64 blocks, and the stride index of the grids
    capped at 1024 x 256 frames (2048 blocks) and at 524,288 frames (4096 blocks)."""
    bad = np.flatnonzero((np.atleast_2d(ref) != np.atleast_2d(got)).any(axis=0))
    if len(bad):
        f = int(bad[0])
        print(f"{what}: {len(bad)} differing frames, first {f} = block {f // B} + {f % B}, group {f // B // GROUP}, "
              f"stride of 262,144 frames {f // 262144}, of 524,288 frames {f // 524288}; max |diff| "
              f"{float(np.nanmax(np.abs(np.atleast_2d(ref)[:, bad].astype(np.float64) - np.atleast_2d(got)[:, bad]))):.3e}")
    assert not len(bad), (what, "first differing frames", bad[:6], "of", len(bad))
    assert ref.shape == got.shape


def block_times(blocks):
    """The block start times as the context accumulates them (AudioContextBase: currentTime += 128 / sr)."""
    out, bt = [], 0.0
    for _ in range(blocks):
        out.append(bt)
        bt = bt + B / SR
    return out


def timeline_at(tl, frames, blocks):
    """Timeline.curve at the chosen frames only (Timeline.curve is a per-sample Python loop)."""
    bt = block_times(blocks)
    return np.array([tl.at(bt[f // B] + (f % B) / SR) for f in frames], F32)


def window_frames(start, stop, blocks):
    """(first frame, end frame) of a scheduled source's window, as ConstantSourceNode.cs:76-141 / OscillatorNode.cs:91-158 compute it
    per block from the accumulated block time."""
    first = end = None
    for b, t0 in enumerate(block_times(blocks)):
        t1 = t0 + B / SR
        if first is None and t1 > start:
            first = b * B + (int(min(max(math.ceil((start - t0) * SR), 0.0), float(B))) if t0 < start < t1 else 0)
        if end is None and not t0 < stop:
            end = b * B
        if end is None and t0 < stop < t1:
            end = b * B + int(min(max(math.floor((stop - t0) * SR), 0.0), float(B)))
    return first, blocks * B if end is None else end


# ---- 1 / 2. OscillatorNode -----------------------------------------------------------------------------------------------------

OSC_FIRST = 301                   # Start(300.2 / SR): the first sample is frame 301
OSC_END = 2190 * B + 17           # Stop at frame 2190 * 128 + 17.5: inside the ragged last group (blocks 2176 .. 2199)
OSC_PIECES = [1000 * B, 1200 * B]   # a cut inside group 15 (block 1000 = 15 * 64 + 40)
OSC_MAX_ABS, OSC_SHARE = 1.2e-7, 1e-3   # the bounds of test_gpu_nodes2.test_oscillator_types_bit_exact
SINE_CLOSED_FORM = 2e-7           # float64 closed form against a float32 sample of a 1-ulp sin


def osc_const(typ):
    """oscillator_kernel: the phase carried serially across 35 groups of 64 blocks (34 full, a ragged one of 24), started and stopped
    at fractional frames."""
    def build(ctx):
        o = OscillatorNode(ctx)
        o.Type = typ
        o.Frequency.Value = 997.0
        o.Connect(ctx.Destination)
        o.Start(300.2 / SR)
        o.Stop((OSC_END + 0.5) / SR)
        return (o,)
    return Scene(f"osc_const_{typ.name}", build, L1, ch=1)


def sine_closed_form(frames):
    n = np.arange(frames, dtype=np.float64)
    want = np.sin(2.0 * np.pi * 997.0 * (n - OSC_FIRST) / SR)
    want[:OSC_FIRST] = 0.0
    want[OSC_END:] = 0.0
    return want


def osc_curve_timeline():
    """Steps and linear ramps only (evaluated in double on both sides): a ramp across the first 14 groups, a step next to block 1024,
    a ramp down through the 2048-block edge, a step in the first block of the ragged group."""
    return (Timeline(440.0, 0.0, NYQ).set(200.0, 0.0).lin(3000.0, 900.37 * T).set(1500.0, at_frame(1024 * B + 3))
            .lin(100.0, 2100 * T).set(800.0, at_frame(2176 * B + 5)))


def osc_curve():
    """oscillator_kernel with a per-sample frequency: the phase increments of 281,600 samples summed across the groups of 64 blocks."""
    def build(ctx):
        o = OscillatorNode(ctx)
        osc_curve_timeline().apply(o.Frequency)
        o.Connect(ctx.Destination)
        o.Start(0.0)
        return (o,)
    return Scene("osc_curve", build, L1, ch=1)


def osc_curve_as_offset():
    """The precondition of osc_curve: its frequency timeline as the output of a ConstantSourceNode (param_curve_kernel)."""
    def build(ctx):
        cs = ConstantSourceNode(ctx)
        osc_curve_timeline().apply(cs.Offset)
        cs.Connect(ctx.Destination)
        cs.Start(0.0)
        return (cs,)
    return Scene("osc_curve_as_offset", build, L1, ch=1)


# ---- 3 / 4 / 5. AudioBufferSourceNode ------------------------------------------------------------------------------------------

LOOP_LEN = B * 37 + 11
LOOP_START, LOOP_END, LOOP_OFFSET = 1000, 3000, 4000   # frames: the start offset lies beyond LoopEnd


def loop_buffer():
    return G.voice(71, LOOP_LEN)


def loop_rate1(window=False):
    """loop_source_kernel: the grid capped at 1024 x 256 frames strides from block 2048 on; the index is taken modulo a loop length
    that is no multiple of the block.  `window`: LoopStart / LoopEnd inside the buffer and a start offset beyond LoopEnd."""
    def build(ctx):
        s = AudioBufferSourceNode(ctx)
        s.Buffer = PlayableAudioBuffer.FromMonoArray(loop_buffer(), SR)
        s.Loop = True
        if window:
            s.LoopStart = (LOOP_START + 0.5) / SR
            s.LoopEnd = (LOOP_END + 0.5) / SR
            s.Start(0.0, (LOOP_OFFSET + 0.5) / SR)
        else:
            s.Start()
        s.Connect(ctx.Destination)
        return (s,)
    return Scene("loop_rate1_window" if window else "loop_rate1", build, L1, ch=1)


def loop_window_indices(blocks):
    """AudioBufferSourceNode.cs:186-235 block by block: a position at or beyond LoopEnd reads from LoopStart, and the position carried
    to the next block is wrapped on its own (so block 0, which starts beyond LoopEnd, reads from LoopStart and block 1 does not
    continue it)."""
    length = LOOP_END - LOOP_START
    idx, p = np.zeros(blocks * B, np.int64), LOOP_OFFSET
    for b in range(blocks):
        pos = LOOP_START if p >= LOOP_END else p
        k = np.arange(B) + pos
        idx[b * B:(b + 1) * B] = np.where(k < LOOP_END, k, LOOP_START + (k - LOOP_END) % length)
        p += B
        if p >= LOOP_END:
            p = LOOP_START + (p - LOOP_END) % length
    return idx


RATE = float(F32(1.37))                      # playbackRate is a float32 parameter
RESAMPLE_END_FRAME = 2100 * B + 60           # the `ends` variant: the buffer runs out inside block 2100
RESAMPLE_END_LEN = int(RESAMPLE_END_FRAME * RATE) + 3
# max |oracle - resample_model| of the scene resample_noloop, all 281,600 frames: measured by
# tests/test_oracle_long_chunks.py::test_resampler_model (x86-64, glibc), 2026-10-19: 6.191e-7 at a peak of 1.14, rounded up here and
# asserted there.  It is the float32 rounding of the oracle's polynomial (intermediate values up to 6) and of its `(float)Pos`;
# tests/test_gpu_long_chunks.py allows 4 x this.
RESAMPLE_MODEL_ERR = 6.2e-7


def resample_buffer(ends=False):
    return G.voice(72, RESAMPLE_END_LEN if ends else 2 * L1 * B)


def resample_noloop(ends=False):
    """resample_fast_kernel: the grid capped at 512 workgroups x 256 samples strides from block 1024 on; with `resample_fast` = 0
    resample_kernel: 35 workgroups of 64 blocks per job, the last one ragged (24 blocks).  `ends`: the buffer runs out inside block
    2100: a partial block with a trajectory entry of its own, then silence."""
    def build(ctx):
        s = AudioBufferSourceNode(ctx)
        s.Buffer = PlayableAudioBuffer.FromMonoArray(resample_buffer(ends), SR)
        s.PlaybackRate.Value = 1.37
        s.Start()
        s.Connect(ctx.Destination)
        return (s,)
    return Scene("resample_ends" if ends else "resample_noloop", build, L1, ch=1)


def resample_model(x, frames, rate=RATE):
    """CubicResampler.cs:26-63 in float64: Catmull-Rom at position 1 + n * rate.  The first four inputs only prime the window
    (tests/test_oracle_dsp.py::test_resampler_first_output_is_second_input_and_linear_is_exact): output 0 is input 1."""
    p = 1.0 + np.arange(frames, dtype=np.float64) * rate
    i = np.floor(p).astype(np.int64)
    t = p - i
    x = x.astype(np.float64)
    s0, s1, s2, s3 = x[i - 1], x[i], x[i + 1], x[i + 2]
    return s1 + t * (0.5 * (s2 - s0) + t * ((s0 - 2.5 * s1 + 2.0 * s2 - 0.5 * s3) + t * (0.5 * (s3 - s0) + 1.5 * (s1 - s2))))


def gsr_loop():
    """gsr_kernel (general replay: looping and resampled): 64 blocks per workgroup from `bl0`, 35 workgroups, the last one ragged,
    its idle waves returning before the barrier."""
    def build(ctx):
        s = AudioBufferSourceNode(ctx)
        s.Buffer = PlayableAudioBuffer.FromMonoArray(G.voice(73, LOOP_LEN), SR)
        s.PlaybackRate.Value = 0.731
        s.Loop = True
        s.Start()
        s.Connect(ctx.Destination)
        return (s,)
    return Scene("gsr_loop", build, L1, ch=1)


# ---- 6 / 7 / 8. DelayNode ------------------------------------------------------------------------------------------------------

DELAY_FRAMES = 14400   # (int)(0.3f * 48000)


def delay_const():
    """delay_kernel: the grid capped at 1024 x 256 frames strides from block 2048 on; a ring of 1 s read 0.3 s back."""
    def build(ctx):
        s = noise(ctx, 1, L1, seed=74)
        d = DelayNode(ctx, 1.0)
        d.DelayTime.Value = 0.3
        s.Connect(d)
        d.Connect(ctx.Destination)
        return (s, d)
    return Scene("delay_const", build, L1, ch=1)


def delay_ramp():
    """delay_kernel with a per-sample delay time (a linear curve: bit-identical on both sides, so (int)(dt * sr) agrees), two channels,
    past the 2048-block grid."""
    def build(ctx):
        s = noise(ctx, 2, L1, seed=75)
        d = DelayNode(ctx, 0.5)
        Timeline(0.0, 0.0, 0.5).set(0.05, 0.0).lin(0.4, L1 * T).apply(d.DelayTime)
        s.Connect(d)
        d.Connect(ctx.Destination)
        return (s, d)
    return Scene("delay_ramp", build, L1, ch=2)


ONSET_ZEROS = 150000           # the delayed buffer's leading exact zeros: 1171 blocks and 112 frames
ONSET_BURST_BLOCK = 1164       # a burst excites the biquad here; it has run out (and the biquad is frozen) before the delay's onset
ONSET_WINDOW = slice(1160 * B, 1200 * B)


def delay_onset(lead=0.0):
    """delay_onset_kernel (option delay_flag_exact): 256 workgroups x 4 waves scan one block each and then stride; the first
    non-zero sample of the delay's output lies in block 1179, beyond the first 1024.  A low-pass biquad (200 Hz, Q 8) behind the delay
    is excited by a burst in blocks 1164 .. 1166 and then frozen with its state by silence (BiQuadFilterNode.cs:103-108) until the
    delay's flag rises: an onset in the wrong block lets it ring in other blocks.  `lead`: what replaces the exact zeros (the control)."""
    def build(ctx):
        x = G.voice(76, L1 * B)
        x[x == 0] = F32(0.125)
        x[:ONSET_ZEROS] = F32(lead)
        late = AudioBufferSourceNode(ctx)
        late.Buffer = PlayableAudioBuffer.FromMonoArray(x, SR)
        d = DelayNode(ctx, 0.05)
        d.DelayTime.Value = 0.02
        lfo = OscillatorNode(ctx)      # a triangle: no sin
        lfo.Type = OscillatorType.Triangle
        lfo.Frequency.Value = 2.0
        depth = GainNode(ctx)
        depth.Gain.Value = 0.005
        lfo.Connect(depth)
        depth.Connect(d.DelayTime)
        burst = AudioBufferSourceNode(ctx)
        burst.Buffer = PlayableAudioBuffer.FromMonoArray(G.voice(77, 3 * B), SR)
        bq = BiQuadFilterNode(ctx)
        bq.Type = FilterType.Lowpass
        bq.Frequency.Value = 200.0
        bq.Q.Value = 8.0
        burst.Connect(bq)
        late.Connect(d)
        d.Connect(bq)
        bq.Connect(ctx.Destination)
        lfo.Start()
        late.Start()
        burst.Start((ONSET_BURST_BLOCK + 0.5) * T)
        return (late, d, lfo, depth, burst, bq)
    return Scene("delay_onset" if lead == 0.0 else "delay_onset_control", build, L1, ch=1)


# ---- 9 / 10. moving parameters held against the double-trig oracle ----------------------------------------------------------------

PAN_LONG_CHANGES = [1023, 1024, 2047, 2048, 2175]   # blocks: on and next to group edges deep in the chunk; 2175 = 33 * 64 + 63, the last block
#                                                     in front of the ragged group (34 * 64 = 2176)


def pan_long_timeline():
    tl = P.ptl().set(-1.0, 0.0).lin(1.0, 300 * T)   # through zero (the stereo law switches sides), across four group edges
    for k, b in enumerate(PAN_LONG_CHANGES):
        tl.set([-0.5, 0.25, -0.75, 0.75, -0.25][k], at_frame(b * B + 17 * (k + 1)))
    return tl.set(0.6, at_frame(2176 * B))          # the first frame of the ragged group


def pan_long(law):
    """stereo_panner_dynamic_kernel: {last pan, gains} handed over through `carry[nb]` across 35 groups of 64 blocks, the last one
    ragged; the pan changes in the blocks around groups 16, 32 and 34."""
    def build(ctx):
        s = noise(ctx, 2 if law == "stereo" else 1, L1, seed=78)
        p = P.panner(ctx, s, pan_long_timeline(), mono=law == "mono")
        p.Connect(ctx.Destination)
        return (s, p)
    return Scene(f"pan_long_{law}", build, L1, ch=2)


PAN_HELD_UNTIL = 2110   # block


def pan_carried_timeline(kind):
    """held: 0.5 through 2110 blocks, written as two events so that the pan is a curve and never changes.  returned: away in block 10,
    back at exactly 0.5 from block 20 on (tests/_param_scenes.pan_quirk_timeline, held from there)."""
    tl = P.ptl().set(0.5, 0.0)
    if kind == "returned":
        tl.set(-0.5, at_frame(10 * B + 17)).set(0.5, at_frame(20 * B + 17))
    return tl.set(0.5, at_frame(1500 * B)).set(-0.25, at_frame(PAN_HELD_UNTIL * B + 17))


def pan_carried(kind, law="quirk"):
    """stereo_panner_dynamic_kernel, where only the carried state tells (see _param_scenes.pan_group_state: under the mono and the
    stereo law the gains are a function of the pan, so a group that lost its state recomputes the right ones).  A mono source into
    the default input: block 0 runs the stereo law on the up-mixed buffer, the later blocks the mono law with the gains in force.
    `held`: the pan never leaves 0.5, so block 0's stereo-law gains have to survive 33 hand-overs from group to group (and the
    one from the job of block 0 through job.state) until block 2110.  `returned`: back at 0.5 with the mono law's gains from block 20 on
    -- the same pan as at the start, other gains.  `law` = 'mono': the comparison render."""
    def build(ctx):
        s = noise(ctx, 1, L1, seed=85)
        p = P.panner(ctx, s, pan_carried_timeline(kind), mono=law == "mono")
        p.Connect(ctx.Destination)
        return (s, p)
    return Scene(f"pan_carried_{kind}" + ("" if law == "quirk" else "_mono"), build, L1, ch=2)


def bq_long():
    """biquad_dynamic_kernel: a peaking section (Q 2, +6 dB) whose frequency ramps from 300 to 5000 Hz over all 2200 blocks, an
    update at every sample, two channels."""
    def build(ctx):
        s = noise(ctx, 2, L1, seed=79)
        bq = P.biquad(ctx, FilterType.Peaking, s, f=P.ftl().set(300.0, 0.0).lin(5000.0, L1 * T), qv=2.0, gv=6.0)
        bq.Connect(ctx.Destination)
        return (s, bq)
    return Scene("bq_long", build, L1, ch=2)


# ---- 11. modulated parameters ----------------------------------------------------------------------------------------------------

def _lfo(ctx, depth):
    """A 3 Hz triangle through a depth gain: no sin, bit-exact."""
    lfo = OscillatorNode(ctx)
    lfo.Type = OscillatorType.Triangle
    lfo.Frequency.Value = 3.0
    g = GainNode(ctx)
    g.Gain.Value = depth
    lfo.Connect(g)
    lfo.Start()
    return lfo, g


def gain_mod():
    """gain_kernel with `curve` and `mod`, and param_mod_kernel (a-rate): grids capped at 1024 x 256 frames, striding from block 2048
    on.  Channel 0: noise through a GainNode whose gain ramps and is modulated; channel 1: a ConstantSourceNode whose offset is
    modulated."""
    def build(ctx):
        lfo, depth = _lfo(ctx, 0.3)
        s = noise(ctx, 1, L1, seed=80)
        g = GainNode(ctx)
        Timeline(1.0).set(0.2, 0.0).lin(0.9, L1 * T).apply(g.Gain)
        depth.Connect(g.Gain)
        s.Connect(g)
        cs = ConstantSourceNode(ctx)
        cs.Offset.Value = 0.1
        depth.Connect(cs.Offset)
        cs.Start()
        mg = ChannelMergerNode(ctx, 2)
        g.Connect(mg, 0, 0)
        cs.Connect(mg, 0, 1)
        mg.Connect(ctx.Destination)
        return (lfo, depth, s, g, cs, mg)
    return Scene("gain_mod", build, L1, ch=2)


def krate_mod(depth=9.0):
    """param_mod_kernel, k-rate (`f - f % 128`), past the 2048-block grid.  ConstantSourceNode.offset is an a-rate parameter and the
    rate of a parameter is fixed by its node, so the k-rate case is the gain (dB) of a peaking biquad, modulated by the same triangle:
    a coefficient update per block, held against the double-trig oracle like every moving biquad.  `depth` 0: the comparison render."""
    def build(ctx):
        lfo, dg = _lfo(ctx, depth)
        s = noise(ctx, 1, L1, seed=81)
        bq = P.biquad(ctx, FilterType.Peaking, s, fv=1200.0, qv=1.5, gv=3.0)
        dg.Connect(bq.Gain)
        bq.Connect(ctx.Destination)
        return (lfo, dg, s, bq)
    return Scene("krate_mod" if depth == 9.0 else "krate_mod_flat", build, L1, ch=1)


# ---- 12 / 17. ConstantSourceNode window and parameter curves -----------------------------------------------------------------------

CONST_START = 0.5
CONST_STOP = (2100 * B + 40.6) / SR


def const_timeline(late=False):
    """Steps and linear ramps, off the sample grid and on block boundaries.  `late`: the events lie in blocks 4090 .. 4150, around the
    4096-block edge of param_curve_kernel's grid."""
    if late:
        return (Timeline(0.25).set(0.5, 0.0).lin(1.0, 4090.37 * T).set(-0.75, at_frame(4095 * B + 127)).set(0.125, at_frame(4096 * B))
                .lin(0.3, 4120.5 * T).set(0.1, at_frame(4140 * B + 3)).lin(-0.4, 4150 * T))
    return (Timeline(0.25).set(0.5, 0.0).lin(1.0, 700.37 * T).set(-0.75, at_frame(1024 * B)).lin(0.3, 2048.5 * T)
            .set(0.1, at_frame(2090 * B + 3)))


def const_window():
    """const_source_kernel and param_curve_kernel: grids capped at 1024 x 256 frames; the window starts at 0.5 s and ends at a
    fractional frame inside block 2100, past the 2048-block stride."""
    def build(ctx):
        cs = ConstantSourceNode(ctx)
        const_timeline().apply(cs.Offset, with_value=True)
        cs.Connect(ctx.Destination)
        cs.Start(CONST_START)
        cs.Stop(CONST_STOP)
        return (cs,)
    return Scene("const_window", build, L1, ch=1)


def param_late():
    """param_curve_kernel past 4096 blocks: the a-rate curve as a ConstantSourceNode's output (channel 0) and as the gain of a GainNode
    on a constant 1 (channel 1); the k-rate sampling of the same timeline is the gain (dB) of a high-shelf biquad on noise (channel 2),
    held against the double-trig oracle."""
    def build(ctx):
        cs = ConstantSourceNode(ctx)
        const_timeline(True).apply(cs.Offset, with_value=True)
        one = ConstantSourceNode(ctx)
        g = GainNode(ctx)
        const_timeline(True).apply(g.Gain, with_value=True)
        one.Connect(g)
        s = noise(ctx, 1, L2, seed=82, scale=0.05)
        tl = const_timeline(True)
        tl.ev = [(k, F32(12.0) * v, t, tc) for k, v, t, tc in tl.ev]   # +-12 dB
        bq = P.biquad(ctx, FilterType.Highshelf, s, g=tl, fv=2000.0, qv=1.2)
        mg = ChannelMergerNode(ctx, 3)
        cs.Connect(mg, 0, 0)
        g.Connect(mg, 0, 1)
        bq.Inputs[0].SetChannelCount(1)
        bq.Connect(mg, 0, 2)
        mg.Connect(ctx.Destination)
        cs.Start()
        one.Start()
        return (cs, one, g, s, bq, mg)
    return Scene("param_late", build, L2, ch=3)


STRIDE = 97   # prime to 128: the strided comparison against Timeline.at visits every frame offset of a block


# ---- 13. AudioStreamSourceNode -------------------------------------------------------------------------------------------------

STREAM_SPEC = [(50000, 1, 44100)] * 6   # 300,000 samples at 44.1 kHz: 326,530 frames at 48 kHz, more than the render


def stream_long(buffers):
    """stream_kernel: 64 blocks per workgroup from `bl0`, 35 workgroups, the last one ragged; the queue hands over from buffer to
    buffer five times inside the chunk.  `buffers`: the builder of tests/test_stream_source.py."""
    def build(ctx):
        s = AudioStreamSourceNode(ctx)
        bufs = buffers(STREAM_SPEC)
        for b in bufs:
            s.QueueBuffer(b)
        s.Connect(ctx.Destination)
        s.Play()
        return (s, bufs)
    return Scene("stream_long", build, L1, ch=2)


# ---- 15 / 16 / 18. buses at L2 ---------------------------------------------------------------------------------------------------

BUS_PAD = 4096


def bus_offset(v, voices):
    """The voice's start offset into its buffer, in frames.  330 voices: anywhere in 0 .. 4095, so the views are unaligned.  40 voices:
    multiples of 4 (16-byte aligned views) except voice 7, whose single odd frame puts the whole bus on the scalar kernel."""
    if voices == 40:
        return (52 * v) % BUS_PAD + (1 if v == 7 else 0)
    return (53 * v + 1) % BUS_PAD


def bus(voices):
    """mix_wide_kernel (330 terms = 5 x 64 + 10, a ragged last batch; the grid of 8192 workgroups x 64 frames strides from frame
    524,288 on) / mix_kernel<1, true> (40 terms, one unaligned view; 2048 x 256 frames, the same edge), and param_curve_kernel for the
    folded gain ramps, which run until blocks 4100 .. 4149.  The voices share three buffers and start at their own offsets; a third
    are plain, a third pass a constant gain, a third a linear gain ramp (the kinds of tests/test_gpu_twin.py)."""
    def build(ctx):
        frames = L2 * B
        bufs = [PlayableAudioBuffer.FromMonoArray(G.voice(90 + k, frames + BUS_PAD), SR) for k in range(3)]
        hold = [bufs]
        for v in range(voices):
            s = AudioBufferSourceNode(ctx)
            s.Buffer = bufs[(v // 3) % 3]
            if v % 3 == 0:
                s.Connect(ctx.Destination)
            else:
                g = GainNode(ctx)
                if v % 3 == 1:
                    g.Gain.Value = 0.1 + 0.001 * v
                else:
                    g.Gain.SetValueAtTime(0.05, 0.0)
                    g.Gain.LinearRampToValueAtTime(0.3, (4100 + v % 50) * T)
                s.Connect(g).Connect(ctx.Destination)
                hold.append(g)
            s.Start(0.0, (bus_offset(v, voices) + 0.5) / SR)
            hold.append(s)
        return tuple(hold)
    return Scene(f"bus_{voices}", build, L2, ch=2)


def downmix_long():
    """downmix_kernel: the grid capped at 2048 x 256 frames strides from frame 524,288 on.  A 2-channel and a 6-channel source into an
    input of exactly one channel."""
    def build(ctx):
        a = noise(ctx, 2, L2 + 2, seed=83)
        b = noise(ctx, 6, L2 + 2, seed=84)
        g = GainNode(ctx)
        g.Gain.Value = 0.6
        g.Inputs[0].SetChannelCount(1)
        g.Inputs[0].SetChannelCountMode(ChannelCountMode.Explicit)
        a.Connect(g)
        b.Connect(g)
        g.Connect(ctx.Destination)
        return (a, b, g)
    return Scene("downmix_long", build, L2, ch=1)


def render_interleaved(mk, scene, channels, opts=None):
    """ProcessBlocksInterleaved of the whole scene in one call (interleave_kernel), returned planar; one chunk on the device."""
    ctx = mk(SR)
    if mk is OfflineAudioContext:
        for k, v in (opts or {}).items():
            ctx.SetOption(k, v)
    ctx.Destination.SetChannelCount(scene.ch)
    hold = scene.build(ctx)
    buf = np.full(scene.frames * channels, 7.0, F32)
    ctx.ProcessBlocksInterleaved(buf, channels, scene.frames // B)
    if mk is OfflineAudioContext:
        assert ctx.GetStats()["chunks"] == 1, (scene.name, ctx.GetStats()["chunks"])
    del hold
    ctx.Dispose()
    return buf.reshape(scene.frames, channels).T.copy()


SCENES = {s.name: s for s in [osc_const(t) for t in OscillatorType] + [
    osc_curve(), osc_curve_as_offset(), loop_rate1(), loop_rate1(True), resample_noloop(), resample_noloop(True), gsr_loop(),
    delay_const(), delay_ramp(), delay_onset(), delay_onset(1e-30), pan_long("stereo"), pan_long("mono"), pan_carried("held"),
    pan_carried("returned"), pan_carried("held", "mono"), pan_carried("returned", "mono"), bq_long(), gain_mod(),
    krate_mod(), const_window(), param_late(), bus(330), bus(40), downmix_long()]}
