"""Scenes of moving parameters, one node kind each, shared by tests/test_oracle_libm_class.py (CPU: the two oracles against each
other) and tests/test_gpu_param_edges.py (the device against both).  A scene is built on any context (HIP product, oracle,
double-trig oracle -- the same host classes); `exact` says whether cosf / sinf / powf and their double-evaluated counterparts agree
on every argument the scene uses, so that the two oracles are bit-equal (asserted in the CPU file) -- scenes of steps, mostly.

Also here: a float64 numpy restatement of AudioParam.ComputeValueAtTime (AudioParam.cs:169-247), written from the C#, which the
tests use to prove on the parameter curve that the edge a scene targets occurs."""
import math

import numpy as np

from graphaudio_amd import (AudioBufferSourceNode, BiQuadFilterNode, ChannelMergerNode, ConstantSourceNode, DelayNode, FilterType,
                            GainNode, OfflineAudioContext, PlayableAudioBuffer, StereoPannerNode)
from tests import _graphs as G

SR = 48000
B = 128
NYQ = SR / 2.0
F32 = np.float32


# ---- AudioParam timeline, float64 restatement ------------------------------------------------------------------------------

class Timeline:
    """The event list of one AudioParam and its value at a time.  Events are (type, value, time, timeConstant) in insertion order of
    AddEvent (:333-352: behind every event with time <= the new one's); values are clamped to [mn, mx] on insertion (:254,268,...)."""

    def __init__(self, value, mn=-np.inf, mx=np.inf):
        self.value, self.mn, self.mx, self.ev = F32(value), mn, mx, []

    def _clamp(self, v):
        v = F32(v)
        return F32(self.mn) if v < self.mn else (F32(self.mx) if v > self.mx else v)

    def _add(self, e):
        lo = 0
        while lo < len(self.ev) and not e[2] < self.ev[lo][2]:
            lo += 1
        self.ev.insert(lo, e)
        return self

    def set(self, v, t):
        return self._add(("set", self._clamp(v), float(t), 0.0))

    def lin(self, v, t):
        return self._add(("lin", self._clamp(v), float(t), 0.0))

    def exp(self, v, t):
        return self._add(("exp", self._clamp(v), float(t), 0.0))

    def target(self, v, t, tc):
        return self._add(("target", self._clamp(v), float(t), float(tc)))

    def cancel(self, t):   # CancelScheduledValues (:312-331)
        self.ev = [e for i, e in enumerate(self.ev) if all(x[2] < t for x in self.ev[:i + 1])]
        return self

    def apply(self, param, with_value=False):
        if with_value:
            param.Value = float(self.value)
        for kind, v, t, tc in self.ev:
            if kind == "set":
                param.SetValueAtTime(float(v), t)
            elif kind == "lin":
                param.LinearRampToValueAtTime(float(v), t)
            elif kind == "exp":
                param.ExponentialRampToValueAtTime(float(v), t)
            else:
                param.SetTargetAtTime(float(v), t, tc)

    @staticmethod
    def _linear(v0, t0, v1, t1, t):   # InterpolateLinear (:220-225)
        u = min(max((t - t0) / (t1 - t0), 0.0), 1.0)
        return F32(float(v0) + float(F32(v1 - v0)) * u)

    @staticmethod
    def _target(e, base, t):          # ComputeSetTargetFromBaseline (:240-247)
        el = t - e[2]
        if el <= 0:
            return base
        tc = max(e[3], 0.001)
        return F32(float(e[1]) + float(F32(base - e[1])) * math.exp(-el / tc))

    def at(self, t):                  # ComputeValueAtTime (:169-217)
        if not self.ev:
            return self.value
        boundary = self.value
        for i, e in enumerate(self.ev):
            if t < e[2]:
                if i == 0:
                    return boundary
                p = self.ev[i - 1]
                if e[0] == "lin":
                    return self._linear(p[1], p[2], e[1], e[2], t)
                if e[0] == "exp":
                    if p[1] <= 0 or e[1] <= 0:
                        return self._linear(p[1], p[2], e[1], e[2], t)
                    u = min(max((t - p[2]) / (e[2] - p[2]), 0.0), 1.0)
                    return F32(float(p[1]) * math.pow(float(F32(e[1] / p[1])), u))
                if p[0] == "target":
                    return self._target(p, boundary, t)
                return p[1]
            if e[0] != "target":
                boundary = e[1]
        last = self.ev[-1]
        return self._target(last, boundary, t) if last[0] == "target" else last[1]

    def curve(self, frames, arate=True, sr=SR):
        """The computed values of `frames` frames from time 0: sampleTime = blockTime + i / sr (:116-120), the block time accumulated
        (AudioContextBase: currentTime += 128 / sr); k-rate samples at the block start (:146)."""
        out = np.zeros(frames, F32)
        bt, dt = 0.0, 1.0 / sr
        for b in range(frames // B):
            for i in range(B):
                out[b * B + i] = self.at(bt + i * dt if arate else bt)
            bt = bt + B / sr
        return out


def biquad_updates(fcurve, qcurve, nch=1):
    """Coefficient updates per block of a non-silent block sequence (BiQuadFilterNode.cs:110-135): usedFreq / usedQ start every
    block at 1000 / 1 and carry from channel to channel; the dirty flag forces the first one."""
    nyq = F32(NYQ)
    counts, dirty = [], True
    for b in range(len(fcurve) // B):
        uf, uq, n = F32(1000.0), F32(1.0), 0
        for _ in range(nch):
            for i in range(B):
                f = min(max(fcurve[b * B + i], F32(1.0)), nyq)
                q = max(F32(0.001), qcurve[b * B + i])
                if dirty or abs(F32(f - uf)) > F32(0.001) or abs(F32(q - uq)) > F32(0.0001):
                    uf, uq, dirty, n = f, q, False, n + 1
        counts.append(n)
    return counts


# ---- rendering ---------------------------------------------------------------------------------------------------------------

class Scene:
    def __init__(self, name, build, blocks, ch=2, exact=False, edits=None, edge=None):
        self.name, self.build, self.frames, self.ch, self.exact = name, build, blocks * B, ch, exact
        self.edits = edits or {}   # frame -> fn(hold): a graph edit between two render calls
        self.edge = edge           # fn(ref): asserts on the oracle's output that the targeted edge occurs
        self.amplified = False     # a resonant section turns one differing coefficient bit into more than the 1e-6 fence

    def __repr__(self):
        return self.name


FORMS = {"default": ([], {}), "chunk5": ([1000, 777, B * 9 + 5, 3001], {"max_chunk_blocks": 5}),
         # chunks of 64 and 76 blocks: the panner's state crosses a chunk boundary (job.state) where the one-piece render crosses a group
         "chunk64": ([B * 64], {"max_chunk_blocks": 129})}
BOTH_FORMS = ["default", "chunk5"]


def render(mk, scene, form="default"):
    pieces, opts = FORMS[form]
    ctx = mk(SR)
    if mk is OfflineAudioContext:
        for k, v in opts.items():
            ctx.SetOption(k, v)
    ctx.Destination.SetChannelCount(scene.ch)
    hold = scene.build(ctx)
    cuts, pos = set(scene.edits), 0
    for p in pieces:
        pos += p
        cuts.add(pos)
    cuts = sorted(c for c in cuts if 0 < c < scene.frames) + [scene.frames]
    out = np.zeros((scene.ch, scene.frames), F32)
    pos = 0
    for c in cuts:
        if pos in scene.edits:
            scene.edits[pos](hold)
        ctx.Render(out, c - pos, pos)
        pos = c
    del hold
    ctx.Dispose()
    return out


def libm_class(a, d):
    """(rms, max-abs, share of differing samples) of two renders."""
    return G.rms(a - d), float(np.abs(a.astype(np.float64) - d).max()), float(np.mean(a != d))


def noise(ctx, nch, blocks, seed=1, start=0.0, duration=None, scale=0.25):
    s = AudioBufferSourceNode(ctx)
    s.Buffer = PlayableAudioBuffer.FromChannelArrays([G.voice(seed + 7 * c, blocks * B, scale) for c in range(nch)], SR)
    if duration is None:
        s.Start(start)
    else:
        s.Start(start, 0.0, duration)
    return s


def at_frame(f, off=0.25):
    """A time between the sample times of frames f-1 and f: the event is seen first by frame f."""
    return (f - 1 + off) / SR if f > 0 else 0.0


# ---- BiQuadFilterNode ----------------------------------------------------------------------------------------------------------

def biquad(ctx, ftype, src, f=None, q=None, g=None, fv=None, qv=None, gv=None):
    bq = BiQuadFilterNode(ctx)
    bq.Type = ftype
    for param, tl, v in ((bq.Frequency, f, fv), (bq.Q, q, qv), (bq.Gain, g, gv)):
        if v is not None:
            param.Value = v
        if tl is not None:
            tl.apply(param)
    src.Connect(bq)
    return bq


def ftl(v=1000.0):
    return Timeline(v, 1.0, NYQ)


def qtl(v=1.0):
    return Timeline(v, 0.001, 1000.0)


def gtl(v=0.0):
    return Timeline(v, -60.0, 60.0)


# Frequency steps, at block starts and mid-block, Q exactly 1.  3000 first; then exactly 1000 (block 4: NO update -- usedFreq
# starts every block at 1000, so the 3000 Hz coefficients stay); 999.9995 / 1000.0009 (inside the 0.001 hysteresis of that baseline:
# still the 3000 Hz coefficients); 1000.002 (outside); Nyquist and 30000 (clamped to Nyquist) for 6 frames each -- a section at
# Nyquist has a double pole at z = -1 and grows like n^1.5 -- entered from a high frequency, where the direct-form-II state is
# small; down in steps to 80, then 1, 0 and -5 (all the lower clamp) and up again.
STEP_F = [(0, 3000.0), (4 * B, 1000.0), (6 * B + 37, 999.9995), (8 * B, 1000.0009), (10 * B + 64, 1000.002), (12 * B, 3500.0),
          (13 * B, 9000.0), (14 * B + 3, NYQ), (14 * B + 9, 12000.0), (16 * B + 100, 30000.0), (16 * B + 106, 6000.0), (17 * B, 1500.0),
          (18 * B, 400.0), (19 * B, 80.0), (21 * B, 1.0), (22 * B + 5, 0.0), (23 * B + 77, -5.0), (25 * B, 20.0), (26 * B, 90.0),
          (27 * B, 440.0), (28 * B + 1, 1000.0), (29 * B + 127, 2500.0)]
STEP_BLOCKS = 32


def step_f_timeline():
    tl = ftl()
    for fr, v in STEP_F:
        tl.set(v, at_frame(fr))
    return tl


def bq_steps(ftype):
    def build(ctx):
        s = noise(ctx, 2, STEP_BLOCKS)
        bq = biquad(ctx, ftype, s, f=step_f_timeline(), gv=6.0)   # (the gain: peaking and the shelves are no identity)
        bq.Connect(ctx.Destination)
        return (s, bq)
    return Scene(f"bq_steps_{ftype.name}", build, STEP_BLOCKS, exact=True)


def ramp_f_timeline(f0, per_sample, blocks, t0=0.0):
    return ftl().set(f0, t0).lin(f0 + per_sample * blocks * B, t0 + blocks * B / SR)


# (name, start, Hz per sample): the update `|f - usedFreq| > 0.001` is a sequential decision every few samples
SLOW_RAMPS = [("slow_0004", 500.0, 0.0004), ("slow_00007", 2200.0, 0.00007), ("exact_001", 512.0, 0.001),
              ("through_1000", 999.9, 0.00003), ("down_0003", 7000.0, -0.0003)]
RAMP_BLOCKS = 50


def bq_slow_ramp(name, f0, slope, ftype=FilterType.Lowpass, nch=2, qv=1.0):
    def build(ctx):
        s = noise(ctx, nch, RAMP_BLOCKS)
        bq = biquad(ctx, ftype, s, f=ramp_f_timeline(f0, slope, RAMP_BLOCKS), qv=qv)
        bq.Connect(ctx.Destination)
        return (s, bq)
    return Scene(f"bq_ramp_{name}_{ftype.name}_{nch}ch", build, RAMP_BLOCKS, ch=max(nch, 2))


def bq_exp_ramp():   # the issue's scene: peaking, Q 4, +9 dB, 150 -> 6000 Hz
    def build(ctx):
        s = noise(ctx, 2, 70)
        bq = biquad(ctx, FilterType.Peaking, s, f=ftl().set(150.0, 0.0).exp(6000.0, 0.15), qv=4.0, gv=9.0)
        bq.Connect(ctx.Destination)
        return (s, bq)
    return Scene("bq_exp_ramp_peaking", build, 70)


Q_STEPS = [(0, 1.00005), (3 * B, 0.99995), (5 * B + 9, 1.0002), (7 * B, 0.0005), (9 * B + 64, -3.0), (11 * B, 2.0), (13 * B + 1, 1.0),
           (15 * B, 0.99985), (17 * B + 50, 700.0), (18 * B, 1.00009)]


def q_step_timeline():
    tl = qtl()
    for fr, v in Q_STEPS:
        tl.set(v, at_frame(fr))
    return tl


def bq_q_steps(ftype):
    """Frequency exactly 1000: only Q decides.  Q within 0.0001 of 1 leaves the coefficients alone."""
    def build(ctx):
        s = noise(ctx, 2, 20)
        pre = biquad(ctx, ftype, s, f=ftl().set(700.0, 0.0).set(1000.0, at_frame(B)), q=q_step_timeline())
        pre.Connect(ctx.Destination)
        return (s, pre)
    return Scene(f"bq_q_steps_{ftype.name}", build, 20, exact=True)


def bq_q_ramp(ftype, with_f):
    """`with_f`: Q up to 8 on a section that moves from 300 to 400 Hz is resonant enough to amplify the last bit of a coefficient
    past the 1e-6 fence of the libm class (1.3e-6 RMS between the two oracles): an "amplified" scene."""
    def build(ctx):
        s = noise(ctx, 2, 40)
        f = ramp_f_timeline(300.0, 0.02, 40) if with_f else None
        bq = biquad(ctx, ftype, s, f=f, fv=None if with_f else 700.0, q=qtl().set(0.5, 0.0).lin(8.0, 30 * B / SR))
        bq.Connect(ctx.Destination)
        return (s, bq)
    sc = Scene(f"bq_q_ramp_{ftype.name}{'_and_f' if with_f else ''}", build, 40, exact=not with_f)   # (fixed frequency: one trig argument)
    sc.amplified = with_f
    return sc


def bq_gain_ramp(ftype, beyond):
    """Gain is k-rate: one value per block, pow(10, gain / 40) per update.  `beyond`: a constant of +/-50 is added through the
    parameter input, so the sum leaves [-60, 60] and is clamped by the parameter."""
    def build(ctx):
        s = noise(ctx, 2, 40, scale=0.002 if beyond else 0.02)   # (+60 dB is a factor of 1000)
        bq = biquad(ctx, ftype, s, fv=1200.0, qv=0.9, g=gtl().set(-30.0, 0.0).lin(30.0, 36 * B / SR))
        hold = [s, bq]
        if beyond:
            cs = ConstantSourceNode(ctx)
            cs.Offset.SetValueAtTime(-50.0, 0.0)
            cs.Offset.SetValueAtTime(50.0, at_frame(20 * B))
            cs.Connect(bq.Gain)
            cs.Start()
            hold.append(cs)
        bq.Connect(ctx.Destination)
        return tuple(hold)
    return Scene(f"bq_gain_ramp_{ftype.name}{'_beyond' if beyond else ''}", build, 40, exact=True)


def bq_channel_carry(nch):
    """1000 Hz at every block start, 2000 Hz from frame 64 of the block on.  Channel 0 starts the block inside the hysteresis of the
    baseline and keeps the 2000 Hz coefficients; channel 1 starts with usedFreq = 2000 carried from channel 0, so it DOES update to
    1000 Hz: the channels are filtered differently in the first half of every block."""
    def build(ctx):
        s = AudioBufferSourceNode(ctx)    # the same noise on every channel: what differs is the filter
        s.Buffer = PlayableAudioBuffer.FromChannelArrays([G.voice(3, 20 * B)] * nch, SR)
        s.Start()
        up = GainNode(ctx)
        up.Gain.Value = 0.5
        s.Connect(up)
        tl = ftl()
        for b in range(20):
            tl.set(1000.0, at_frame(b * B)).set(2000.0, at_frame(b * B + 64))
        bq = biquad(ctx, FilterType.Bandpass, up, f=tl)
        bq.Connect(ctx.Destination)
        return (s, up, bq)
    return Scene(f"bq_channel_carry_{nch}ch", build, 20, ch=max(nch, 2), exact=True)


def bq_mono_becomes_stereo():
    def build(ctx):
        m = noise(ctx, 1, 40, seed=5)
        st = noise(ctx, 2, 40, seed=9, start=at_frame(17 * B))
        mix = GainNode(ctx)
        mix.Gain.Value = 0.7
        m.Connect(mix)
        st.Connect(mix)
        bq = biquad(ctx, FilterType.Highpass, mix, f=ramp_f_timeline(800.0, 0.0005, 40), qv=2.0)
        bq.Connect(ctx.Destination)
        return (m, st, mix, bq)
    return Scene("bq_mono_becomes_stereo", build, 40, exact=True)


TYPE_EDITS = [(6 * B, FilterType.Highpass), (1000 + 777, FilterType.Peaking), (20 * B + 7, FilterType.Notch), (30 * B, FilterType.Lowshelf)]


def bq_type_written():
    """The Type setter between render pieces while the frequency is automated: _coefficientsDirty forces an update at the next
    sample even where the frequency sits inside the hysteresis (the plateau at exactly 1000 Hz from block 18 on)."""
    def build(ctx):
        s = noise(ctx, 2, 40)
        bq = biquad(ctx, FilterType.Lowpass, s, f=ftl().set(400.0, 0.0).lin(1000.0, 18 * B / SR), qv=1.0, gv=6.0)
        bq.Connect(ctx.Destination)
        return (s, bq)

    def setter(t):
        def fn(hold):
            hold[1].Type = t
        return fn
    return Scene("bq_type_written", build, 40, edits={fr: setter(t) for fr, t in TYPE_EDITS})


def bq_automation_ends_and_returns(upto=2):
    """moving -> constant (the Value setter cancels the timeline: the static cascade kernels take over the state) -> moving again."""
    def build(ctx):
        s = noise(ctx, 2, 60)
        bq = biquad(ctx, FilterType.Peaking, s, f=ramp_f_timeline(300.0, 0.05, 20), qv=3.0, gv=8.0)
        bq.Connect(ctx.Destination)
        return (s, bq)

    def constant(hold):
        hold[1].Frequency.Value = 620.0

    def again(hold):
        hold[1].Frequency.SetValueAtTime(620.0, 40 * B / SR)
        hold[1].Frequency.LinearRampToValueAtTime(200.0, 55 * B / SR)
        hold[1].Q.SetValueAtTime(3.0, 42 * B / SR)
        hold[1].Q.LinearRampToValueAtTime(0.7, 50 * B / SR)
    edits = {15 * B + 40: constant, 36 * B: again}
    return Scene("bq_automation_ends_and_returns", build, 60, exact=True, edits={k: edits[k] for k in list(edits)[:upto]})


def bq_input_falls_silent():
    """The source ends after block 12 and another starts in block 25; the frequency keeps ramping: no processing, no coefficient
    update and a frozen state in between (BiQuadFilterNode.cs:103-108)."""
    def build(ctx):
        a = noise(ctx, 2, 13, seed=2)
        b = noise(ctx, 2, 40, seed=4, start=at_frame(25 * B + 30))
        bq = biquad(ctx, FilterType.Bandpass, a, f=ramp_f_timeline(250.0, 0.3, 45), qv=6.0)
        b.Connect(bq)
        bq.Connect(ctx.Destination)
        return (a, b, bq)
    return Scene("bq_input_falls_silent", build, 45)


def modulator_signal(n, seed, period=600.0):
    return (np.sin(2 * np.pi * np.arange(n) / period) + 0.3 * G.voice(seed, n)).astype(F32)


def modulator(ctx, n, depth, seed, period=600.0, loop=False, nan_at=(), hold_at=()):
    """`nan_at`: frames that hold NaN; `hold_at`: frames (ascending) that repeat the value of the frame before them."""
    m = AudioBufferSourceNode(ctx)
    x = modulator_signal(n, seed, period)
    for i in nan_at:
        x[i] = np.nan
    for i in hold_at:
        x[i] = x[i - 1]
    m.Buffer = PlayableAudioBuffer.FromMonoArray(x, SR)
    m.Loop = loop
    g = GainNode(ctx)
    g.Gain.Value = depth
    m.Connect(g)
    m.Start()
    return m, g


def bq_modulated():
    """Frequency and Q modulated at audio rate by buffers that end mid-chunk (frames 3,333 and 2,100): from the next block on the
    parameters are their intrinsic values again."""
    def build(ctx):
        s = noise(ctx, 2, 45)
        bq = biquad(ctx, FilterType.Lowpass, s, fv=1500.0, qv=2.0)
        mf = modulator(ctx, 3333, 900.0, 41)
        mq = modulator(ctx, 2100, 1.5, 43, period=333.0)
        mf[1].Connect(bq.Frequency)
        mq[1].Connect(bq.Q)
        bq.Connect(ctx.Destination)
        return (s, bq) + mf + mq
    return Scene("bq_modulated", build, 45)


CROWD_TYPES = list(FilterType)[:8]


def bq_crowd_timelines(v):
    """(frequency timeline, Q timeline) of voice v, one of them None."""
    if v % 3 == 0:
        return ftl().set(200.0 + 37.0 * v, 0.0).set(1000.0, at_frame((3 + v % 5) * B + v)).set(150.0 + 11 * v, at_frame(14 * B + 3 * v)), None
    if v % 3 == 1:
        return ramp_f_timeline(300.0 + 50.0 * v, 0.0004 * (1 + v % 4), 24), None
    return None, qtl().set(0.5 + 0.05 * v, 0.0).lin(4.0, (10 + v % 9) * B / SR)


def bq_crowd():
    """80 automated biquads in one level (the kernel's second wave of 64 one-lane jobs), all filter types, steps / ramps / Q ramps;
    voice v lands on channel v % 32 of a 32-channel destination."""
    def build(ctx):
        mg = ChannelMergerNode(ctx, 32)
        hold = [mg]
        for v in range(80):
            s = noise(ctx, 1, 24, seed=100 + v)
            f, q = bq_crowd_timelines(v)
            bq = biquad(ctx, CROWD_TYPES[v % 8], s, f=f, q=q, fv=None if f else 900.0 + 13 * v, gv=float(v % 13 - 6))
            bq.Inputs[0].SetChannelCount(1)
            bq.Connect(mg, 0, v % 32)
            hold += [s, bq]
        mg.Connect(ctx.Destination)
        return tuple(hold)
    return Scene("bq_crowd", build, 24, ch=32)


NAN_Q_FRAMES = (300, 301, 900, 2000)


def bq_nan_q(moving_f, held=False):
    """Q modulated by a buffer that holds NaN at chosen frames.  Math.Max(0.001f, NaN) is NaN (BiQuadFilterNode.cs:124):
    `|q - usedQ| > 0.0001` is false, so with the frequency held the NaN frames change nothing; with the frequency moving the
    update at such a frame makes every coefficient NaN, and the state, and so every sample after it."""
    def build(ctx):
        s = noise(ctx, 2, 24)
        f = ramp_f_timeline(400.0, 0.01, 24) if moving_f else None
        bq = biquad(ctx, FilterType.Lowpass, s, f=f, fv=None if moving_f else 1800.0, qv=2.0)
        m = modulator(ctx, 24 * B, 0.5, 47, **{"hold_at" if held else "nan_at": NAN_Q_FRAMES})
        m[1].Connect(bq.Q)
        bq.Connect(ctx.Destination)
        return (s, bq) + m
    return Scene(f"bq_nan_q_{'moving' if moving_f else 'held'}_f{'_no_nan' if held else ''}", build, 24)


NAN_F_FRAMES = (500, 1700)


def bq_nan_f(held=False):
    """A NaN frequency: Math.Clamp keeps it; `|f - usedFreq| > 0.001` is false, nothing updates, the frames pass with the old
    coefficients (usedFreq is not touched) -- unless Q moves at that frame: then the coefficients are NaN.  `held`: the same scene
    with the value of the frame before in place of each NaN (f == usedFreq: no update either)."""
    def build(ctx):
        s = noise(ctx, 2, 24)
        bq = biquad(ctx, FilterType.Highpass, s, fv=2500.0, qv=1.5)
        m = modulator(ctx, 24 * B, 300.0, 49, **{"hold_at" if held else "nan_at": NAN_F_FRAMES})
        m[1].Connect(bq.Frequency)
        bq.Connect(ctx.Destination)
        return (s, bq) + m
    return Scene(f"bq_nan_f{'_no_nan' if held else ''}", build, 24)


NAN_Q_SET_AT = 4 * B


def bq_constant_nan_q(freq, behind_convolver=False, with_nan=True):
    """A CONSTANT NaN Q, written by the Value setter (its Math.Clamp keeps it) between two render calls, after four blocks at Q 2
    (which use up the dirty flag): the constant-coefficient path, evaluated on the host.  At 1000 Hz nothing updates any more
    (`|NaN - 1| > 0.0001` is false, the frequency sits on the baseline): the Q 2 coefficients stay, the render equals the one without
    the write (`with_nan` False).  At any other frequency the next block's first sample updates and every coefficient is NaN.
    `behind_convolver`: the planner also looks at the coefficients of a constant biquad behind a convolver."""
    def build(ctx):
        from graphaudio_amd import ConvolverNode
        s = noise(ctx, 2, 12)
        node, hold = s, []
        if behind_convolver:
            cv = ConvolverNode(ctx)
            cv.Buffer = PlayableAudioBuffer.FromChannelArrays([G.synth_ir(c, 300) for c in range(2)], SR)
            s.Connect(cv)
            node, hold = cv, [cv]
        bq = biquad(ctx, FilterType.Lowpass, node, fv=freq, qv=2.0)
        bq.Connect(ctx.Destination)
        return tuple([s, bq] + hold)

    def write(hold):
        hold[1].Q.Value = float("nan")
    return Scene(f"bq_constant_nan_q_{int(freq)}{'_behind_convolver' if behind_convolver else ''}{'' if with_nan else '_not_written'}", build, 12,
                 edits={NAN_Q_SET_AT: write} if with_nan else None)


# ---- StereoPannerNode --------------------------------------------------------------------------------------------------------

def ptl(v=0.0):
    return Timeline(v, -1.0, 1.0)


def panner(ctx, src, tl=None, value=None, mono=False):
    p = StereoPannerNode(ctx)
    if mono:
        p.Inputs[0].SetChannelCount(1)
    if value is not None:
        p.Pan.Value = value
    if tl is not None:
        tl.apply(p.Pan)
    src.Connect(p)
    return p


PAN_STEPS = [(0, -1.0), (2 * B, -0.5), (4 * B + 33, 0.0), (6 * B, 0.5), (8 * B + 1, 1.0), (10 * B, 1.5), (12 * B + 127, -2.0),
             (14 * B, 0.0), (15 * B + 64, 0.25), (17 * B, -0.25), (19 * B, 0.75)]


def pan_step_timeline():
    tl = ptl()
    for fr, v in PAN_STEPS:
        tl.set(v, at_frame(fr))
    return tl


def pan_steps(law):
    """law: 'stereo' (2-channel source), 'mono' (input limited to one channel: the mono law from the first block), 'quirk' (a mono
    source into the default input: block 0 runs the stereo law on the up-mixed buffer, later blocks the mono law)."""
    def build(ctx):
        s = noise(ctx, 2 if law == "stereo" else 1, 22)
        p = panner(ctx, s, pan_step_timeline(), mono=law == "mono")
        p.Connect(ctx.Destination)
        return (s, p)
    return Scene(f"pan_steps_{law}", build, 22, exact=True)


def pan_ramp(law):
    """A ramp through 0 (the stereo law switches sides there), held, then a ramp back to exactly the held value of before."""
    def build(ctx):
        s = noise(ctx, 2 if law == "stereo" else 1, 70)
        tl = ptl().set(-1.0, 0.0).lin(1.0, 0.15).set(1.0, 60 * B / SR).lin(0.4, 64 * B / SR).set(0.4, 66 * B / SR)
        p = panner(ctx, s, tl, mono=law == "mono")
        p.Connect(ctx.Destination)
        return (s, p)
    return Scene(f"pan_ramp_{law}", build, 70)


PAN_GROUP_CHANGES = [63, 64, 65, 127, 128]


def pan_group_edges(law):
    """The pan holds for many blocks and changes (mid-block) exactly in blocks 63, 64, 65, 127 and 128 of the render: in one chunk
    those straddle the kernel's groups of 64 blocks."""
    def build(ctx):
        s = noise(ctx, 2 if law == "stereo" else 1, 140)
        tl = ptl().set(0.5, 0.0)
        for k, b in enumerate(PAN_GROUP_CHANGES):
            tl.set([-0.5, 0.25, -0.75, 0.75, -0.25][k], at_frame(b * B + 17 * (k + 1)))
        p = panner(ctx, s, tl, mono=law == "mono")
        p.Connect(ctx.Destination)
        return (s, p)
    return Scene(f"pan_group_edges_{law}", build, 140, exact=True)


# (block, pan): 0.5 from the start, away and BACK to 0.5 inside the first group, 0.5 again in front of the third
PAN_QUIRK_CHANGES = [(10, -0.5), (20, 0.5), (66, 0.25), (100, 0.5), (131, -0.25)]


def pan_quirk_timeline():
    tl = ptl().set(0.5, 0.0)
    for b, v in PAN_QUIRK_CHANGES:
        tl.set(v, at_frame(b * B + 17))
    return tl


def pan_group_state(law="quirk"):
    """Where the gains are NOT a function of the pan: a mono source into the default input.  Block 0 runs the stereo law on the
    up-mixed buffer; the later blocks run the mono law and keep block 0's gains until the pan changes.  The pan leaves 0.5 in block
    10 and is back at exactly 0.5 from block 20 on, now with the mono law's gains: the state at the start of the per-sample job
    (last pan 0.5, stereo-law gains) and the state at the end of its first group of 64 blocks (last pan 0.5, mono-law gains) have the
    same pan and different gains, and no pan change in blocks 65 (66 in one piece) recomputes them.  Only the carried state tells;
    the same holds in front of the third group (0.5 again from block 100 to 131).  `law` = 'mono': the comparison render."""
    def build(ctx):
        s = noise(ctx, 1, 140)
        p = panner(ctx, s, pan_quirk_timeline(), mono=law == "mono")
        p.Connect(ctx.Destination)
        return (s, p)
    return Scene(f"pan_group_state_{law}", build, 140, exact=True)


def pan_crowd_timeline(v):
    tl = ptl().set(-1.0 + v / 40.0, 0.0)
    if v % 3 == 0:
        return tl.lin(1.0 - v / 40.0, (6 + v % 11) * B / SR)
    return tl.set(0.9 - v / 50.0, at_frame((2 + v % 7) * B + v)).set(-0.3 + v / 200.0, at_frame(12 * B + 5 * v))


def pan_crowd():
    def build(ctx):
        hold = []
        for v in range(80):
            s = noise(ctx, 1 + v % 2, 20, seed=300 + v)
            p = panner(ctx, s, pan_crowd_timeline(v), mono=v % 4 == 0)
            g = GainNode(ctx)
            g.Gain.Value = 0.125
            p.Connect(g).Connect(ctx.Destination)
            hold += [s, p, g]
        return tuple(hold)
    return Scene("pan_crowd", build, 20)


# ---- the scene families of the libm class ------------------------------------------------------------------------------------

def biquad_scenes():
    sc = [bq_steps(t) for t in CROWD_TYPES]
    sc += [bq_slow_ramp(*r) for r in SLOW_RAMPS]
    sc += [bq_slow_ramp("slow_0004", 500.0, 0.0004, FilterType.Peaking, nch=3, qv=2.0), bq_slow_ramp("through_1000", 999.9, 0.00003, FilterType.Allpass, nch=3),
           bq_exp_ramp()]
    sc += [bq_q_steps(t) for t in (FilterType.Lowpass, FilterType.Notch, FilterType.Highshelf)]
    sc += [bq_q_ramp(FilterType.Bandpass, False), bq_q_ramp(FilterType.Lowpass, True)]
    sc += [bq_gain_ramp(t, beyond) for t in (FilterType.Peaking, FilterType.Lowshelf, FilterType.Highshelf) for beyond in (False, True)]
    sc += [bq_channel_carry(2), bq_channel_carry(3), bq_mono_becomes_stereo(), bq_type_written(), bq_automation_ends_and_returns(),
           bq_input_falls_silent(), bq_modulated(), bq_crowd()]
    return sc


def panner_scenes():
    sc = [pan_steps(law) for law in ("stereo", "mono", "quirk")]
    sc += [pan_ramp(law) for law in ("stereo", "mono")]
    sc += [pan_group_edges(law) for law in ("stereo", "mono")] + [pan_group_state()]
    return sc + [pan_crowd()]


def nan_scenes():
    return [bq_nan_q(False), bq_nan_q(True), bq_nan_f(), bq_constant_nan_q(1000.0), bq_constant_nan_q(1800.0),
            bq_constant_nan_q(1800.0, behind_convolver=True)]


# ---- DelayNode with a moving delayTime (no libm: the plain oracle is the reference) ---------------------------------------------

def delay_samples(curve):
    """delayTime * sampleRate as the node computes it: float * int -> float (DelayNode.cs:66,86), before the (int) truncation."""
    return curve.astype(F32) * F32(SR)


def integer_distance(prod):
    """Distance of every product from the nearest integer, 0 where it sits exactly on one."""
    p = prod.astype(np.float64)
    return np.abs(p - np.rint(p))


def dtl(max_delay):
    return Timeline(0.0, 0.0, max_delay)


def delay_timeline(kind, max_delay):
    """Steps land on n + 0.5 samples, ramps move by half a sample per frame between n + 0.25 and n + 0.75: (int)(delayTime * sr)
    never comes within 1e-3 of deciding differently (asserted by the tests on the float32 curve)."""
    tl = dtl(max_delay)
    top = max_delay * SR
    if kind == "steps":      # 0, then steps; beyond maxDelayTime (clamped on insertion), exactly maxDelayTime, across the write position
        pts = [(0, 0.0), (3 * B, 10.5), (5 * B + 7, 0.0), (6 * B, top * 2), (8 * B + 64, 3.5), (10 * B, top), (12 * B + 1, 127.5),
               (13 * B, 128.5), (14 * B + 100, top - 0.5), (16 * B, 1.5)]
        for fr, d in pts:
            tl.set(d / SR, at_frame(fr))
    else:                    # ramps up and down at half a sample per frame
        lo, n = 20.25, int(min(top - 40, 600))
        tl.set(lo / SR, 0.0).lin((lo + n / 2) / SR, n / SR).set((lo + n / 2) / SR, 8 * B / SR).lin(lo / SR, (8 * B + n) / SR)
    return tl


def delay_scene(kind, max_delay, nch, negative_mod=False):
    def build(ctx):
        s = noise(ctx, nch, 24, seed=60 + nch)
        d = DelayNode(ctx, max_delay)
        delay_timeline(kind, max_delay).apply(d.DelayTime)
        hold = [s, d]
        if negative_mod:     # intrinsic + modulation < 0 from block 4 to block 9: clamped to 0 by the parameter
            cs = ConstantSourceNode(ctx)
            cs.Offset.SetValueAtTime(0.0, 0.0)
            cs.Offset.SetValueAtTime(-1.0, at_frame(4 * B + 9))
            cs.Offset.SetValueAtTime(0.0, at_frame(9 * B + 3))
            cs.Connect(d.DelayTime)
            cs.Start()
            hold.append(cs)
        g = GainNode(ctx)
        g.Gain.Value = 0.8
        s.Connect(d)
        d.Connect(g).Connect(ctx.Destination)
        return tuple(hold + [g])
    return Scene(f"delay_{kind}_{max_delay}_{nch}ch{'_negmod' if negative_mod else ''}", build, 24, ch=max(nch, 2), exact=True)


# (chunk5 renders in chunks of 640 frames: a ring of 0.005 s = 240 frames is shorter, one of 0.05 s = 2,400 frames longer)
DELAY_CASES = [("steps", 0.005, 1, False), ("steps", 0.05, 2, False), ("steps", 0.05, 3, True), ("ramps", 0.005, 2, False),
               ("ramps", 0.05, 1, True), ("ramps", 0.05, 3, False)]


# ---- parameter timelines, observed through ConstantSourceNode.offset (channel 0) and GainNode.gain on a constant 1 (channel 1) ----

FMAX = float(np.finfo(F32).max)

T = B / SR
# name -> (timeline maker, has exp / pow curves).  Event times off the sample grid, on block boundaries, two at the same time; a
# ramp inserted in front of an event scheduled earlier; the reference's special cases of exponential ramps (from / to zero, across a
# sign: linear); SetTargetAtTime with a time constant of 0 (0.001 is used).  The late_* timelines are the bases of PARAM_EDITS.
PARAM_TIMELINES = {
    "steps_and_linear": (lambda: Timeline(0.25, -FMAX, FMAX).set(0.5, 0.0).set(-0.75, 2 * T).set(0.125, 2 * T).lin(1.0, 3.37 * T)
                         .lin(-1.0, 6 * T).set(0.3, 6 * T).lin(0.9, 6.0001 * T).lin(0.1, 30 * T), False),
    "ramp_inserted_in_front": (lambda: Timeline(0.1, -FMAX, FMAX).set(1.0, 5 * T).lin(2.0, 1 * T).lin(-2.0, 9.5 * T), False),
    "exp_ramps": (lambda: Timeline(0.2, -FMAX, FMAX).set(0.01, 0.0).exp(1.0, 4.3 * T).exp(0.05, 9 * T).set(0.0, 10 * T).exp(0.7, 13 * T)
                  .set(-0.5, 14 * T).exp(0.5, 17 * T).exp(3.0, 40 * T), True),
    "set_target": (lambda: Timeline(0.0, -FMAX, FMAX).set(1.0, 0.0).target(0.2, 1.5 * T, 0.004).set(0.6, 8 * T).target(-1.0, 10 * T, 0.0)
                   .target(0.5, 14.25 * T, 0.02), True),
    "late_base_ramp": (lambda: Timeline(0.1, -FMAX, FMAX).set(0.5, 0.0).lin(1.0, 20.5 * T), False),
    "late_base_step": (lambda: Timeline(0.1, -FMAX, FMAX).set(0.5, 0.0), False),
    "late_base_exp": (lambda: Timeline(0.2, -FMAX, FMAX).set(0.4, 0.0).exp(2.0, 20.5 * T), True),
}
PARAM_BLOCKS = 24
LATE = 10 * B + 50   # the frame of the edit: between two render calls, inside block 10; "now" is the start of block 11
# name -> (base timeline, frame of the edit, operations).  cancel_*: CancelScheduledValues inside a ramp.  late_*: a ramp whose END
# (3 blocks) lies before "now" (11 blocks) is scheduled between two render calls: the event lands in the part of the list the
# render has passed.  With a later event behind it, the curve from the next block on runs from the late event's value and time to
# that event (a jump); as the last event, its value holds from the next block on (a jump).
PARAM_EDITS = {
    "cancel_linear": ("steps_and_linear", LATE, [("cancel", 20 * T)]),
    "cancel_exp": ("exp_ramps", 20 * B, [("cancel", 25 * T)]),
    "late_linear_ramp_in_front_of_a_ramp": ("late_base_ramp", LATE, [("lin", -0.7, 3 * T)]),
    "late_linear_ramp_as_last_event": ("late_base_step", LATE, [("lin", 0.9, 3 * T)]),
    "late_exp_ramp_in_front_of_an_exp_ramp": ("late_base_exp", LATE, [("exp", 0.05, 3 * T)]),
    "late_exp_ramp_as_last_event": ("late_base_step", LATE, [("exp", 0.02, 3.3 * T)]),
    "late_exp_then_linear": ("late_base_ramp", LATE, [("exp", 0.25, 2 * T), ("lin", -0.5, 4.5 * T)]),
}


def param_has_exp(name, edit=None):
    return PARAM_TIMELINES[edit and PARAM_EDITS[edit][0] or name][1] or bool(edit and any(op[0] == "exp" for op in PARAM_EDITS[edit][2]))


def param_scene(name, edit=None):
    """The curve itself is the output.  `edit`: a key of PARAM_EDITS (its base timeline replaces `name`)."""
    frame, ops = None, []
    if edit:
        name, frame, ops = PARAM_EDITS[edit]
    mk, _ = PARAM_TIMELINES[name]

    def build(ctx):
        cs = ConstantSourceNode(ctx)
        mk().apply(cs.Offset, with_value=True)
        one = ConstantSourceNode(ctx)
        g = GainNode(ctx)
        mk().apply(g.Gain, with_value=True)
        mg = ChannelMergerNode(ctx, 2)
        cs.Connect(mg, 0, 0)
        one.Connect(g)
        g.Connect(mg, 0, 1)
        mg.Connect(ctx.Destination)
        cs.Start()
        one.Start()
        return (cs, g, one, mg)

    def do_edit(hold):
        for param in (hold[0].Offset, hold[1].Gain):
            for op in ops:
                if op[0] == "cancel":
                    param.CancelScheduledValues(op[1])
                elif op[0] == "lin":
                    param.LinearRampToValueAtTime(op[1], op[2])
                else:
                    param.ExponentialRampToValueAtTime(op[1], op[2])
    return Scene(f"param_{edit or name}", build, PARAM_BLOCKS, exact=True, edits={frame: do_edit} if edit else None)


def param_expected(name, frames, edit=None):
    """The float64 restatement's curve.  An edit between two render calls is seen from the next block on: the block under way is
    computed."""
    if not edit:
        return PARAM_TIMELINES[name][0]().curve(frames)
    name, frame, ops = PARAM_EDITS[edit]
    tl = PARAM_TIMELINES[name][0]()
    cut = -(-frame // B) * B
    head = tl.curve(frames)[:cut]
    for op in ops:
        if op[0] == "cancel":
            tl.cancel(op[1])
        else:
            getattr(tl, op[0])(op[1], op[2])
    return np.concatenate([head, tl.curve(frames)[cut:]])
