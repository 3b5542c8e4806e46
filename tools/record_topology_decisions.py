#!/usr/bin/env python3
"""What the graph analysis of a chunk decides, seen from outside (tools/record_topology_decisions.py OUT.json): every scene below is
rendered on the device in one call and again in three uneven pieces, and per scene and way the record keeps the counters the
decisions move (blocks_rendered, chunks, segments, kernel_launches, delay_flags_read, delay_flags_predicted) and the SHA-256 of the
output samples.  Only the public API and the scene builders of the test modules are used, so the file runs unchanged on any commit
that has those modules: tests/golden/topology_decisions.json was written by it on the commit BEFORE the analysis moved into
ga_topology.cpp, and tests/test_gpu_topology_record.py compares a fresh record with it."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from graphaudio_amd import DelayNode, GainNode, OfflineAudioContext

SR = 48000
COUNTERS = ("blocks_rendered", "chunks", "segments", "kernel_launches", "delay_flags_read", "delay_flags_predicted")
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
    out = np.zeros((ch, frames), np.float32)
    pos = 0
    for p in list(pieces or []) + [frames]:
        p = min(p, frames - pos)
        if p > 0:
            ctx.Render(out, p, pos)
            pos += p
    st = ctx.GetStats()
    del hold
    ctx.Dispose()
    return out, st


def record(with_samples=False):
    rec, samples = {}, {}
    for name, scene in scenes().items():
        for way, pieces in (("one_call", None), ("three_pieces", PIECES)):
            out, st = render(scene, pieces)
            entry = {k: int(st[k]) for k in COUNTERS}
            entry["sha256"] = hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest()
            entry["rms"] = float(np.sqrt(np.mean(out.astype(np.float64) ** 2)))
            rec[f"{name}/{way}"] = entry
            samples[f"{name}/{way}"] = out
    return (rec, samples) if with_samples else rec


if __name__ == "__main__":
    text = json.dumps(record(), indent=1, sort_keys=True) + "\n"
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w", encoding="utf-8") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
