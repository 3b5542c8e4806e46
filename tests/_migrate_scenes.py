"""Edit sessions for option "conv_migrate" (DESIGN.md 2b): a ConvolverNode renders for a while, then an edit puts something behind it
that amplifies or quantises last-bit differences -- a DelayNode.delayTime, a resonant low biquad, a feedback loop with a gain near 1.
With `coarse_min_blocks = 1` the convolver starts on formulation D (9,000 taps: P = 71, the smallest class that takes D, and C / R
after the move); the option moves it to formulation R in the chunk after the edit.

A scene is a builder `build(ctx) -> Session`; the same builder runs on the oracle and on the device.  `run(ctx, scene)` renders the
pieces in front of the edit, calls `edit()`, renders the rest, and returns the output with the statistics after each half.

In every scene the convolver also feeds the destination: a node that nothing reachable from the destination listens to is not
processed at all (pull model), so a convolver wired to the sink alone would not run -- and keep no state -- before the edit.
"""
import numpy as np

from graphaudio_amd import (AudioBufferSourceNode, BiQuadFilterNode, ConvolverNode, DelayNode, FilterType, GainNode,
                            PlayableAudioBuffer)
from tests import _graphs as G

SR = 48000
TAPS = 9000          # P = 71
BASE_DELAY = 0.004   # DelayNode.delayTime in front of the modulation, seconds
DEPTH = 0.02


class Session:
    def __init__(self, channels, edit, depth=None):
        self.channels = channels
        self.edit = edit          # the edit between the two halves
        self.depth = depth        # the gain whose output drives a delayTime after the edit (None: another kind of sink)


class Scene:
    def __init__(self, name, build, pre=(30,), post=(40, 20), opts=None):
        self.name = name
        self.build = build
        self.pre = tuple(pre)      # render calls in front of the edit, in blocks
        self.post = tuple(post)    # ... and behind it
        self.opts = dict(opts or {})   # device options of this scene (besides coarse_min_blocks / conv_migrate / max_chunk_blocks)

    @property
    def pre_frames(self):
        return 128 * sum(self.pre)

    @property
    def frames(self):
        return 128 * (sum(self.pre) + sum(self.post))


def run(ctx, scene, probe=False):
    """-> (output [channels][frames], statistics after the first half, at the end); `probe`: only the depth signal reaches the
    destination (the oracle's view of what drives the delay time)"""
    ses = scene.build(ctx, probe=probe)
    out = np.zeros((ses.channels, scene.frames), np.float32)
    pos = 0
    for n in scene.pre:
        ctx.Render(out, 128 * n, pos)
        pos += 128 * n
    st0 = ctx.GetStats() if hasattr(ctx, "GetStats") else None
    ses.edit()
    for n in scene.post:
        ctx.Render(out, 128 * n, pos)
        pos += 128 * n
    st1 = ctx.GetStats() if hasattr(ctx, "GetStats") else None
    return out, st0, st1


def _source(ctx, arrays, when=0.0, start=True):
    s = AudioBufferSourceNode(ctx)
    s.Buffer = PlayableAudioBuffer.FromChannelArrays(list(arrays), SR) if len(arrays) > 1 else PlayableAudioBuffer.FromMonoArray(arrays[0], SR)
    if start:
        s.Start(when)
    return s


def _ir(channels, taps=TAPS):
    return PlayableAudioBuffer.FromChannelArrays([G.synth_ir(c, taps) for c in range(channels)], SR)


def _delay_sink(ctx, frames, out, voice=6):
    """a dry voice through a DelayNode whose delayTime the edit will modulate; -> (delay, depth gain)"""
    v = _source(ctx, [G.voice(voice, frames)])
    d = DelayNode(ctx, 0.05)
    d.DelayTime.Value = BASE_DELAY
    depth = GainNode(ctx)
    depth.Gain.Value = DEPTH
    if out is not None:
        v.Connect(d).Connect(out)
    return d, depth


def delay_time_scene(name, *, src_channels=1, ir_channels=2, taps=TAPS, gain_front=False, source_when=0.0, source_blocks=None,
                     second_source_when=None, swap_to_stereo=False, vibrato=False, pre=(30,), post=(40, 20), opts=None):
    """test_gpu_reforder's `delay_time` scene as an edit session: depth.Connect(d.DelayTime) is made between two renders."""
    total = 128 * (sum(pre) + sum(post))

    def build(ctx, probe=False):
        ctx.Destination.SetChannelCount(2)
        n = 128 * source_blocks if source_blocks else total
        s = _source(ctx, [G.voice(5 + 20 * c, n) for c in range(src_channels)], when=source_when)
        cv = ConvolverNode(ctx)
        cv.Buffer = _ir(ir_channels, taps)
        head = s
        if gain_front:
            g = GainNode(ctx)
            g.Gain.Value = 0.5
            head = s.Connect(g)
        head.Connect(cv)
        if second_source_when is not None:   # (the first source has ended: this one makes the sink audible behind the edit)
            _source(ctx, [G.voice(77, total)], when=second_source_when).Connect(cv)
        d, depth = _delay_sink(ctx, total, None if probe else ctx.Destination)
        cv.Connect(depth)
        if vibrato and not probe:
            # a voice whose playbackRate a signal modulates makes every chunk a two-stage chunk; behind a gain of exactly 0 it adds
            # exact zeros to the bus, so the output is the convolver's and the delayed voice's share, value for value
            from tests._fuzz import rate_modulator
            vs = _source(ctx, [G.voice(90, total)], start=False)
            rate_modulator(ctx, np.random.default_rng(7), vs, total / SR)
            mute = GainNode(ctx)
            mute.Gain.Value = 0.0
            vs.Connect(mute).Connect(ctx.Destination)
            vs.Start()
        if probe:
            depth.Connect(ctx.Destination)
        else:
            cv.Connect(ctx.Destination)

        def edit():
            if not probe:
                depth.Connect(d.DelayTime)
            if swap_to_stereo:   # the two input channels of the convolver start to differ
                s.Disconnect()
                s2 = _source(ctx, [G.voice(41, total), G.voice(42, total)], when=ctx.CurrentTime)
                s2.Connect(g if gain_front else cv)
        return Session(2, edit, depth)
    return Scene(name, build, pre, post, opts)


PEAK = dict(type=FilterType.Peaking, f=104.0, q=2.1, gain=6.0)   # fuzz graph 22879: 2.6e-5 in round 3 behind a convolver


def _set_biquad(bq, type, f, q, gain):
    bq.Type = type
    bq.Frequency.Value = f
    bq.Q.Value = q
    bq.Gain.Value = gain


def group_scene(name, *, sink, voices=9, target=4, taps=TAPS, bus_to_destination=True, sink_from_start=False, pre=(40,), post=(40, 20)):
    """`voices` convolvers share one impulse response, each into one bus gain (a pre-mixed group of formulation D), and a dry voice
    runs through a DelayNode.  sink = "delay": after the edit convolver `target` also drives that delay's delayTime through a depth
    gain; sink = "biquad": a fresh resonant biquad is inserted between the bus and the destination."""
    total = 128 * (sum(pre) + sum(post))

    def build(ctx, probe=False):
        ctx.Destination.SetChannelCount(2)
        ir = _ir(2, taps)
        bus = GainNode(ctx)
        bus.Gain.Value = 0.5
        cvs = []
        for v in range(voices):
            s = _source(ctx, [G.voice(v, total)])
            cv = ConvolverNode(ctx)
            cv.Buffer = ir
            s.Connect(cv).Connect(bus)
            cvs.append(cv)
        d, depth = _delay_sink(ctx, total, None if probe else ctx.Destination, voice=60)
        if probe:
            cvs[target].Connect(depth)
            depth.Connect(ctx.Destination)
            return Session(2, lambda: None, depth)
        if bus_to_destination or sink == "biquad":
            bus.Connect(ctx.Destination)
        else:   # the bus stays processed (and the group pre-mixed) but only the delayed voice is heard
            mute = GainNode(ctx)
            mute.Gain.Value = 0.0
            bus.Connect(mute).Connect(ctx.Destination)

        def edit():
            if sink == "delay":
                cvs[target].Connect(depth)
                depth.Connect(d.DelayTime)
            else:
                bq = BiQuadFilterNode(ctx)
                _set_biquad(bq, **PEAK)
                bus.Disconnect()
                bus.Connect(bq).Connect(ctx.Destination)
        if sink_from_start:   # (the twin of a session whose node cannot be put on R by an option alone)
            edit()
            return Session(2, lambda: None, depth if sink == "delay" else None)
        return Session(2, edit, depth if sink == "delay" else None)
    return Scene(name, build, pre, post)


def retune_scene(name="retune", pre=(30,), post=(40, 20)):
    """a gentle low-pass behind one convolver from the start; between two renders it is written to the resonant peaking setting"""
    total = 128 * (sum(pre) + sum(post))

    def build(ctx, probe=False):
        ctx.Destination.SetChannelCount(2)
        s = _source(ctx, [G.voice(5, total)])
        cv = ConvolverNode(ctx)
        cv.Buffer = _ir(2)
        bq = BiQuadFilterNode(ctx)
        _set_biquad(bq, FilterType.Lowpass, 4000.0, 0.7, 0.0)
        s.Connect(cv).Connect(bq).Connect(ctx.Destination)
        return Session(2, lambda: _set_biquad(bq, **PEAK))
    return Scene(name, build, pre, post)


def loop_scene(name="loop", pre=(40,), post=(40, 20)):
    """convolver -> sum gain -> DelayNode(0.02 s) -> gain 0.8 -> sum gain: the last connection closes the loop behind the running node"""
    total = 128 * (sum(pre) + sum(post))

    def build(ctx, probe=False):
        ctx.Destination.SetChannelCount(2)
        s = _source(ctx, [G.voice(5, total)])
        cv = ConvolverNode(ctx)
        cv.Buffer = _ir(2)
        mix = GainNode(ctx)
        d = DelayNode(ctx, 0.05)
        d.DelayTime.Value = 0.02
        fb = GainNode(ctx)
        fb.Gain.Value = 0.8
        s.Connect(cv).Connect(mix).Connect(ctx.Destination)
        mix.Connect(d).Connect(fb)
        return Session(2, lambda: fb.Connect(mix))
    return Scene(name, build, pre, post)


BASE = delay_time_scene("base")
HISTORY_SHAPES = [
    delay_time_scene("long_first_render", pre=(300,)),               # longer than the 128-block history: the double buffer has turned over
    delay_time_scene("uneven_first_render", pre=(7, 19, 4)),
    delay_time_scene("gain_in_front", gain_front=True),              # the node's own history copy instead of a zero-copy span
    delay_time_scene("no_ext_history", opts={"coarse_ext_history": 0}),
    delay_time_scene("stereo_source", src_channels=2),               # two different channels into a two-channel response (bShared false)
    delay_time_scene("mono_then_stereo", swap_to_stereo=True),       # bShared true, and the channels diverge with the edit
    delay_time_scene("true_stereo", src_channels=2, ir_channels=4),  # (L,h0)(L,h1)(R,h2)(R,h3)
]
EMPTY_HISTORIES = [
    delay_time_scene("source_starts_after_the_edit", source_when=128 * 34 / SR),        # 4 blocks behind the edit
    # silent for 200 blocks in front of the edit (the history is all zeros, but not flagged empty); a second source starts 4 blocks behind it
    delay_time_scene("source_ended_long_before", source_blocks=40, second_source_when=128 * 244 / SR, pre=(240,)),
]
BASE_WITH_VIBRATO = delay_time_scene("base_next_to_a_vibrato_voice", vibrato=True)
LONG_IR = delay_time_scene("more_than_1024_partitions", src_channels=1, ir_channels=1, taps=128 * 1100 + 17, pre=(25,), post=(35,))
GROUP_MEMBER = [group_scene("member_4_leaves", sink="delay", target=4), group_scene("leader_leaves", sink="delay", target=0)]
GROUP_MEMBER_ALONE = [group_scene("member_4_leaves_delay_alone", sink="delay", target=4, bus_to_destination=False),
                      group_scene("leader_leaves_delay_alone", sink="delay", target=0, bus_to_destination=False)]
GROUP_ALL = group_scene("all_members_at_once", sink="biquad")
RETUNE = retune_scene()
LOOP = loop_scene()
# formulation A: nine voices share a 3,000-tap response (P = 24); the twin has voice 0's sink from the first block
A_TAPS = 3000
A_MEMBER = group_scene("formulation_a_member", sink="delay", target=0, taps=A_TAPS)
A_MEMBER_TWIN = group_scene("formulation_a_member_sink_from_start", sink="delay", target=0, taps=A_TAPS, sink_from_start=True)

DELAY_SCENES = [BASE, BASE_WITH_VIBRATO] + HISTORY_SHAPES + EMPTY_HISTORIES + [LONG_IR] + GROUP_MEMBER + GROUP_MEMBER_ALONE + [A_MEMBER]
ALL_SCENES = DELAY_SCENES + [GROUP_ALL, RETUNE, LOOP]


def delay_indices(scene, depth_signal):
    """(int)(delayTime * sampleRate) of every post-edit sample, as DelayNode computes it (DelayNode.cs:66,86): the parameter's value is
    the intrinsic value plus the mono down-mix of what is connected to it"""
    post = depth_signal[:, scene.pre_frames:]
    mod = post.mean(axis=0, dtype=np.float32) if post.shape[0] > 1 else post[0]
    t = np.clip(np.float32(BASE_DELAY) + mod.astype(np.float32), np.float32(0), np.float32(0.05))
    return (t * np.float32(SR)).astype(np.int32)
