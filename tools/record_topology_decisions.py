#!/usr/bin/env python3
"""What the planner of a chunk decides, seen from outside (tools/record_topology_decisions.py OUT.json [topology|conv]): every scene of
a table below is rendered on the device in one call and again in three uneven pieces, and per scene and way the record keeps the
counters the decisions move and the SHA-256 of the output samples.  Only the public API and the scene builders of the test modules
are used, so the file runs unchanged on any commit that has those modules.

Table "topology" (scenes(), COUNTERS): the graph analysis.  tests/golden/topology_decisions.json was written on the commit BEFORE the
analysis moved into ga_topology.cpp, and tests/test_gpu_topology_record.py compares a fresh record with it.

Table "conv" (conv_scenes(), CONV_COUNTERS): the fine-partition side of the convolver planner (ga_plan_conv.cpp) -- shared-IR groups
of formulation A, private impulse responses on formulations B, C and R, the shared -> private history hand-down and the conv_migrate
rebuild.  tests/golden/conv_plan_decisions.json was written on the commit BEFORE the private-IR stage was split into passes, and
tests/test_gpu_conv_plan_record.py compares a fresh record with it."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from graphaudio_amd import AudioBufferSourceNode, ConvolverNode, DelayNode, GainNode, OfflineAudioContext, PlayableAudioBuffer

SR = 48000
COUNTERS = ("blocks_rendered", "chunks", "segments", "kernel_launches", "delay_flags_read", "delay_flags_predicted")
CONV_COUNTERS = ("blocks_rendered", "chunks", "segments", "kernel_launches", "mac_launches", "mac_flops_total", "mac_bytes_total",
                 "ref_order_rows", "conv_migrations", "n_conv_rows")
PIECES = [128 * 7 + 5, 128 * 11 - 3]   # ... and the rest: three uneven pieces


def _two_gains(ctx):
    """tests/test_gpu_cycles.py::test_two_gains_feeding_each_other_one_block_feedback"""
    from tests import test_gpu_cycles as C
    s = C.src(ctx, 2, 128 * 40, stereo=True)
    g1, g2 = GainNode(ctx), GainNode(ctx)
    g1.Gain.Value = 0.5
    g2.Gain.Value = 0.9
    s.Connect(g1)
    g1.Connect(g2)
    g2.Connect(g1)
    g2.Connect(ctx.Destination)
    return [s, g1, g2]


def _two_loops_uncut(ctx):
    """tests/test_gpu_cycles.py::test_two_loops_with_different_delays_and_one_that_cannot_be_cut, kind "uncut\""""
    from tests import test_gpu_cycles as C
    s = C.src(ctx, 30, 128 * 40, stereo=True)
    bus = GainNode(ctx)
    bus.Gain.Value = 0.7
    s.Connect(bus)
    hold = [s, bus]
    for i, dt in enumerate((0.03, 0.071)):
        d = DelayNode(ctx, 0.5)
        d.DelayTime.Value = dt
        fb = GainNode(ctx)
        fb.Gain.Value = 0.4 + 0.1 * i
        bus.Connect(d)
        d.Connect(fb).Connect(d)
        d.Connect(ctx.Destination)
        hold += [d, fb]
    a, c = GainNode(ctx), GainNode(ctx)
    a.Gain.Value = 0.5
    c.Gain.Value = 0.5
    bus.Connect(a).Connect(c).Connect(a)
    c.Connect(ctx.Destination)
    bus.Connect(ctx.Destination)
    return hold + [a, c]


def _spatial(ctx):
    from tests import test_gpu_spatial as S
    from tests import test_gpu_spatial_signals as SS
    nb = 60
    return SS.move_scene(ctx, SS.move_input(nb, False), S.noise_set(SS.MOVE_A * SS.MOVE_E, SS.MOVE_T, 77), nb)


def _fuzz(seed, frames):
    def build(ctx):
        from tests._fuzz import build_random_graph
        return build_random_graph(ctx, seed, frames)   # (the destination's channel count)
    return build


def scenes():
    """name -> (builder, frames, channels or None = what the builder returns, options)"""
    from tests import test_gpu_cycles as C
    from tests import test_gpu_delay_flag_exact as E
    from tests import test_gpu_delay_flag_loops as L
    from tests import test_gpu_rate_mod_cycles as R
    long, short = 128 * 300, E.FRAMES
    return {
        "echo_0.0123": (lambda ctx: C._echo(ctx, 0.0123, long), long, 2, {}),
        "echo_0.25": (lambda ctx: C._echo(ctx, 0.25, long), long, 2, {}),
        "two_gains": (_two_gains, 128 * 40, 2, {}),
        "two_loops_uncut": (_two_loops_uncut, 128 * 120, 2, {}),
        "vibrato_echo": (R.vibrato_echo, long, 2, {}),
        "cone_loop_tap": (R.cone_loop("tap"), long, 2, {}),
        "base_z805_value_1": (lambda ctx: E.base_scene(ctx, kind="z805"), short, 1, {"delay_flag_exact": 1}),
        "two_delays_value_1": (lambda ctx: E.two_delays(ctx, "z805"), short, 1, {"delay_flag_exact": 1}),
        "loop_scene_d_value_2": (lambda ctx: L.loop_scene(ctx, tap="d"), short, 1, {"delay_flag_exact": 2}),
        "loop_scene_d_conv_value_2": (lambda ctx: L.loop_scene(ctx, tap="d", conv=True), short, 1, {"delay_flag_exact": 2}),
        "closed_through_a_finished_node_value_2": (L.closed_through_a_finished_node, short, 1, {"delay_flag_exact": 2}),
        "spatial_signals": (_spatial, 128 * 60, 2, {"spatial_param_signals": 1}),
        "fuzz_50003": (_fuzz(50003, 128 * 36), 128 * 36, None, {"max_chunk_blocks": 11, "coarse_min_blocks": 1 << 30}),
    }


class Edit:
    """what a builder returns when the graph is edited between two render calls: `fn()` runs when `frame` frames are rendered"""
    def __init__(self, frame, fn, hold):
        self.frame, self.fn, self.hold = frame, fn, hold


def _voice_into(ctx, cv, seeds, frames, when=0.0):
    """a source of len(seeds) channels -> cv, started at `when` seconds"""
    from tests import _graphs as G
    s = AudioBufferSourceNode(ctx)
    arrays = [G.voice(v, frames + 256) for v in seeds]
    s.Buffer = PlayableAudioBuffer.FromChannelArrays(arrays, SR) if len(arrays) > 1 else PlayableAudioBuffer.FromMonoArray(arrays[0], SR)
    s.Connect(cv)
    s.Start(when)
    return s


def _convolver(ctx, channels, taps, seed0):
    from tests import _graphs as G
    cv = ConvolverNode(ctx)
    cv.Buffer = PlayableAudioBuffer.FromChannelArrays([G.synth_ir(c, taps, seed0=seed0) for c in range(channels)], SR)
    cv.Connect(ctx.Destination)
    return cv


MID_CHUNK = 128 * 5.5 / SR   # inside the first chunk of every scene below: the segment views of that input disagree


def _conv_shared(frames):
    """formulation A: eight mono voices on one shared 2-channel response of 300 taps (P = 3), voice 3 started in the middle of a chunk"""
    def build(ctx):
        from tests import _graphs as G
        ir = PlayableAudioBuffer.FromChannelArrays([G.synth_ir(c, 300) for c in range(2)], SR)
        hold = []
        for v in range(8):
            cv = ConvolverNode(ctx)
            cv.Buffer = ir
            cv.Connect(ctx.Destination)
            hold += [cv, _voice_into(ctx, cv, [v], frames, MID_CHUNK if v == 3 else 0.0)]
        return hold
    return build


def _conv_private(frames, taps_list, kinds=("mono", "stereo", "true_stereo", "mid_chunk")):
    """private responses, per tap count: a mono input into 2 channels (one x-row), a stereo input into 2 channels, a true-stereo
    node (4-channel response, stereo input), and a node whose source starts in the middle of a chunk"""
    def build(ctx):
        hold = []
        for i, taps in enumerate(taps_list):
            for j, kind in enumerate(kinds):
                seed = 100 + 40 * i + 10 * j
                cv = _convolver(ctx, 4 if kind == "true_stereo" else 2, taps, seed)
                seeds = [seed] if kind in ("mono", "mid_chunk") else [seed, seed + 1]
                hold += [cv, _voice_into(ctx, cv, seeds, frames, MID_CHUNK if kind == "mid_chunk" else 0.0)]
        return hold
    return build


def _conv_17_channels(frames):
    """a mono input into a 17-channel response: 17 columns on one x-row, two sets"""
    def build(ctx):
        cv = _convolver(ctx, 17, 200, 300)
        return [cv, _voice_into(ctx, cv, [7], frames)]
    return build


def _conv_reforder(frames):
    """tests/test_gpu_reforder.py::test_true_stereo_and_private_impulse_responses_bit_equal"""
    def build(ctx):
        from tests import _graphs as G
        hold = []
        for v in range(3):
            s = AudioBufferSourceNode(ctx)
            s.Buffer = PlayableAudioBuffer.FromChannelArrays([G.voice(10 * v, frames), G.voice(10 * v + 1, frames)], SR)
            cv = ConvolverNode(ctx)
            cv.Buffer = PlayableAudioBuffer.FromChannelArrays([G.synth_ir(c, 700 + 4000 * v, seed0=50 + 10 * v) for c in range(4)], SR)
            s.Connect(cv).Connect(ctx.Destination)
            s.Start(0.01 * v)
            hold += [s, cv]
        return hold
    return build


def _conv_hand_down(frames, edit_frame):
    """a mono source into a 2-channel response; between two render calls a stereo source joins it and the channels start to differ"""
    def build(ctx):
        cv = _convolver(ctx, 2, 128 * 17 - 5, 400)
        hold = [cv, _voice_into(ctx, cv, [21], frames)]

        def edit():
            hold.append(_voice_into(ctx, cv, [22, 23], frames, edit_frame / SR))
        return Edit(edit_frame, edit, hold)
    return build


def _conv_migrate(ctx):
    """tests/_migrate_scenes.py BASE: a convolver on formulation D starts to drive a delay time and moves to formulation R"""
    from tests import _migrate_scenes as M
    ses = M.BASE.build(ctx)
    return Edit(M.BASE.pre_frames, ses.edit, ses)


def conv_scenes():
    """as scenes(); every scene spans at least three chunks, so the x-plane pair alternates and the history comes from the previous pair"""
    from tests import _migrate_scenes as M
    n, chunks = 128 * 40, {"max_chunk_blocks": 11}
    c_opts = dict(chunks, coarse=0)
    return {
        "a_shared_ir": (_conv_shared(n), n, 2, chunks),
        "b_private_p1_p2_p17": (_conv_private(n, (100, 200, 128 * 17 - 5)), n, 2, chunks),
        "b_17_channels": (_conv_17_channels(n), n, 17, chunks),
        "c_p65_radix16_mixed": (_conv_private(n, (8320,), ("mono", "true_stereo")), n, 2, c_opts),
        "c_p65_radix2": (_conv_private(n, (8320,), ("mono", "true_stereo")), n, 2, dict(c_opts, tconv_radix16=0)),
        "r_true_stereo_and_private": (_conv_reforder(128 * 80), 128 * 80, 2, {"conv_reference_order": 2, "max_chunk_blocks": 23}),
        "hand_down_mono_then_stereo": (_conv_hand_down(n, 128 * 15), n, 2, chunks),
        "migrate_base": (_conv_migrate, M.BASE.frames, 2, {"max_chunk_blocks": 37, "coarse_min_blocks": 1, "conv_migrate": 1}),
    }


def render(scene, pieces):
    build, frames, ch, opts = scene
    ctx = OfflineAudioContext(SR)
    for k, v in opts.items():
        ctx.SetOption(k, v)
    if ch is not None:
        ctx.Destination.SetChannelCount(ch)
    hold = build(ctx)
    if ch is None:
        ch = hold
    edit = hold if isinstance(hold, Edit) else None
    out = np.zeros((ch, frames), np.float32)
    pos = 0
    for p in list(pieces or []) + [frames]:
        end = min(pos + p, frames)
        while pos < end:   # (a call ends where the graph is edited)
            stop = edit.frame if edit and pos < edit.frame < end else end
            ctx.Render(out, stop - pos, pos)
            pos = stop
            if edit and pos == edit.frame:
                edit.fn()
    st = ctx.GetStats()
    del hold
    ctx.Dispose()
    return out, st


def record(with_samples=False, table=scenes, counters=COUNTERS):
    rec, samples = {}, {}
    for name, scene in table().items():
        for way, pieces in (("one_call", None), ("three_pieces", PIECES)):
            out, st = render(scene, pieces)
            entry = {k: int(st[k]) for k in counters}
            entry["sha256"] = hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest()
            entry["rms"] = float(np.sqrt(np.mean(out.astype(np.float64) ** 2)))
            rec[f"{name}/{way}"] = entry
            samples[f"{name}/{way}"] = out
    return (rec, samples) if with_samples else rec


if __name__ == "__main__":
    conv = len(sys.argv) > 2 and sys.argv[2] == "conv"
    text = json.dumps(record(table=conv_scenes, counters=CONV_COUNTERS) if conv else record(), indent=1, sort_keys=True) + "\n"
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w", encoding="utf-8") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
