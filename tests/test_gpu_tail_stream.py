"""The coarse stage of a chunk on a second stream, beside the next chunk's upload and pre-mix (option coarse_tail_stream).

An asynchronous render into page-locked rows whose chunk is table upload + one pre-mix launch + forward / sum / inverse runs the
three transforms on a second stream; the next chunk's upload and pre-mix do not wait for them, everything else on the context's
stream does (Context::joinTail).  Whatever runs where, every step has to arrive bit for bit as a blocking render of the same step
produces it (the yardstick of tests/test_gpu_async_host.py).  The sequences below are the places where something else than that
upload + pre-mix pair follows a tail: reading the rows back, rows that are reused, renders of several chunks, an edit of the
graph, the option switched, a blocking render, the context disposed with work in flight, a sharded render.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch

from graphaudio_amd import AudioBufferSourceNode, ConvolverNode, OfflineAudioContext, PlayableAudioBuffer
from graphaudio_amd.distributed import init_sharded
from tests import _graphs as G

SR = 48000
FRAMES = 128 * 300
VOICES = 12
TAPS = 20000
STEPS = 5


def build(ctx, total=FRAMES * STEPS):
    """config3_convolver, keeping the convolvers: (channels, convolvers)"""
    ir = PlayableAudioBuffer.FromChannelArrays([G.synth_ir(c, TAPS) for c in range(2)], SR)
    ctx.Destination.SetChannelCount(2)
    cvs = []
    for v in range(VOICES):
        s = AudioBufferSourceNode(ctx)
        s.Buffer = PlayableAudioBuffer.FromMonoArray(G.voice(v, total + 256), SR)
        cv = ConvolverNode(ctx)
        cv.Buffer = ir
        s.Connect(cv).Connect(ctx.Destination)
        s.Start()
        cvs.append(cv)
    return 2, cvs


def pinned():
    return torch.zeros((2, FRAMES), dtype=torch.float32).pin_memory()


def context(**opts):
    ctx = OfflineAudioContext(SR)
    ctx.SetOption("coarse_min_blocks", 1)
    for k, v in opts.items():
        ctx.SetOption(k, v)
    return ctx


def blocking(steps=STEPS, between=None, **opts):
    """the yardstick: one blocking render per step into pageable rows"""
    ctx = context(**opts)
    _, cvs = build(ctx)
    outs = []
    for k in range(steps):
        if between:
            between(ctx, cvs, k)
        a = np.zeros((2, FRAMES), np.float32)
        ctx.Render(a, FRAMES)
        outs.append(a)
    ctx.Dispose()
    assert all(G.rms(o) > 1e-4 for o in outs)
    return outs


_ref = {}


def reference():
    if "plain" not in _ref:
        _ref["plain"] = blocking()
    return _ref["plain"]


def test_steps_into_rows_of_their_own():
    ref = reference()
    ctx = context()
    build(ctx)
    ctx.SetOption("async", 1)
    rows = [pinned() for _ in range(STEPS)]
    for k in range(STEPS):
        ctx.Render(rows[k].numpy(), FRAMES)
    ctx.Synchronize()
    st = ctx.GetStats()
    assert st["deferred_handovers"] == STEPS - 1
    for k in range(STEPS):
        assert np.array_equal(ref[k], rows[k].numpy()), k
    ctx.Dispose()


@pytest.mark.parametrize("synchronize", [True, False])
def test_steps_into_the_same_rows(synchronize):
    ref = reference()
    ctx = context()
    build(ctx)
    ctx.SetOption("async", 1)
    row = pinned()
    for k in range(STEPS):
        ctx.Render(row.numpy(), FRAMES)
        if synchronize:
            ctx.Synchronize()
            assert np.array_equal(ref[k], row.numpy()), k
    ctx.Synchronize()
    assert np.array_equal(ref[STEPS - 1], row.numpy())   # (hand-overs into the same rows arrive in the order of the steps)
    if not synchronize:
        assert ctx.GetStats()["deferred_handovers"] == STEPS - 1
    ctx.Dispose()


def test_renders_of_several_chunks():
    ref = blocking(steps=3, max_chunk_blocks=64)
    ctx = context(max_chunk_blocks=64)
    build(ctx)
    ctx.SetOption("async", 1)
    rows = [pinned() for _ in range(3)]
    for k in range(3):
        ctx.Render(rows[k].numpy(), FRAMES)
    ctx.Synchronize()
    for k in range(3):
        assert np.array_equal(ref[k], rows[k].numpy()), k
    ctx.Dispose()


def test_a_voice_disconnected_between_two_steps():
    def edit(ctx, cvs, k):
        if k == 2:
            cvs[3].Disconnect()

    ref = blocking(between=edit)
    ctx = context()
    _, cvs = build(ctx)
    ctx.SetOption("async", 1)
    rows = [pinned() for _ in range(STEPS)]
    for k in range(STEPS):
        edit(ctx, cvs, k)
        ctx.Render(rows[k].numpy(), FRAMES)
    ctx.Synchronize()
    assert not np.array_equal(ref[2], reference()[2])   # (the edit is audible)
    for k in range(STEPS):
        assert np.array_equal(ref[k], rows[k].numpy()), k
    ctx.Dispose()


def test_the_option_switched_off_and_on_between_steps():
    ref = reference()
    ctx = context()
    build(ctx)
    ctx.SetOption("async", 1)
    rows = [pinned() for _ in range(STEPS)]
    for k in range(STEPS):
        if k == 1:
            ctx.SetOption("coarse_tail_stream", 0)
        if k == 3:
            ctx.SetOption("coarse_tail_stream", 1)
        ctx.Render(rows[k].numpy(), FRAMES)
    ctx.Synchronize()
    assert ctx.GetStats()["deferred_handovers"] == STEPS - 1
    for k in range(STEPS):
        assert np.array_equal(ref[k], rows[k].numpy()), k
    ctx.Dispose()
    off = context(coarse_tail_stream=0)   # ... and never on: the schedule of one stream
    build(off)
    off.SetOption("async", 1)
    for k in range(STEPS):
        off.Render(rows[k].numpy(), FRAMES)
    off.Synchronize()
    assert off.GetStats()["deferred_handovers"] == STEPS - 1
    for k in range(STEPS):
        assert np.array_equal(ref[k], rows[k].numpy()), k
    off.Dispose()


def test_a_blocking_render_after_two_asynchronous_ones():
    ref = reference()
    ctx = context()
    build(ctx)
    ctx.SetOption("async", 1)
    rows = [pinned() for _ in range(2)]
    for k in range(2):
        ctx.Render(rows[k].numpy(), FRAMES)
    ctx.SetOption("async", 0)
    a = np.zeros((2, FRAMES), np.float32)
    ctx.Render(a, FRAMES)
    for k in range(2):
        assert np.array_equal(ref[k], rows[k].numpy()), k
    assert np.array_equal(ref[2], a)
    ctx.Dispose()


def test_dispose_without_a_final_synchronize():
    ref = reference()
    ctx = context()
    build(ctx)
    ctx.SetOption("async", 1)
    rows = [pinned() for _ in range(3)]
    for k in range(3):
        ctx.Render(rows[k].numpy(), FRAMES)
    ctx.Dispose()   # waits for what is in flight; the last step's rows were never handed over
    for k in range(2):
        assert np.array_equal(ref[k], rows[k].numpy()), k
    again = context()   # ... and the next context finds the device in order
    build(again)
    again.SetOption("async", 1)
    row = pinned()
    again.Render(row.numpy(), FRAMES)
    again.Synchronize()
    assert np.array_equal(ref[0], row.numpy())
    again.Dispose()


def test_sharded_renders_on_one_rank():
    ref = reference()
    ctx = context()
    build(ctx)
    init_sharded(ctx, 0, 1)
    ctx.SetOption("async", 1)
    rows = [pinned() for _ in range(4)]
    ctx.Render(rows[0].numpy(), FRAMES)   # (a plain render in front: its tail is on the second stream when the sharded one starts)
    for k in range(1, 4):
        ctx.RenderReduce(rows[k].numpy(), FRAMES)
    ctx.Synchronize()
    for k in range(4):
        assert np.array_equal(ref[k], rows[k].numpy()), k
    ctx.CommDestroy()
    ctx.Dispose()
