"""The pre-mix launch is sized to the chip, not to the chunk (option coarse_premix_wgs_per_cu, ga_coarse.hip::coarse_premix_kernel).

Every summing job gets R x compute units / summing jobs workgroups; workgroup i walks an equal share of the job's 16-byte words in
steps of 64 words and masks the last step.  The additions of a frame are the ones the kernel made when a workgroup was 256 frames
of the chunk, in the same order, so the renders below have to be BIT FOR BIT what the library rendered before the grid changed:
tests/golden/premix_grid_parent.npz holds, per case, the SHA-256 of the float32 output of that library (equal digests <=> equal
arrays) and every 8th sample of it (np.array_equal on those says where a difference is).  The same renders stay within 1e-5 RMS of
the CPU oracle.

Cases: member counts (9: the smallest pre-mixed group here; 65: two descriptor batches and uneven wave shares; 130) x chunk lengths
(128 x 3: fewer words than workgroups; 128 x 259: shares that are no multiple of 64 words; 128 x 260), members whose `in` is not
16-byte aligned (looping voices that start and loop 3 samples into their buffers), members with `carry` terms (node outputs, two
chunks without carried tails: the second chunk reads the histories the first one wrote, and has two summing jobs), each at
R = 1, 3 and 7.
"""
import hashlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from graphaudio_amd import AudioBufferSourceNode, ConvolverNode, GainNode, OfflineAudioContext, PlayableAudioBuffer
from tests import _graphs as G
from tests._oracle import OracleContext

SR = 48000
TAPS = 20000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "premix_grid_parent.npz")
F259 = 128 * 259


def _looping_unaligned(ctx, frames):
    ir = PlayableAudioBuffer.FromChannelArrays([G.synth_ir(c, TAPS) for c in range(2)], SR)
    ctx.Destination.SetChannelCount(2)
    for v in range(9):
        s = AudioBufferSourceNode(ctx)
        s.Buffer = PlayableAudioBuffer.FromMonoArray(G.voice(v, frames + 3), SR)
        s.Loop = True
        s.LoopStart = 3.0 / SR
        cv = ConvolverNode(ctx)
        cv.Buffer = ir
        s.Connect(cv).Connect(ctx.Destination)
        s.Start(0.0, 3.0 / SR)
    return 2


def _behind_gains(ctx, frames):
    ir = PlayableAudioBuffer.FromChannelArrays([G.synth_ir(c, TAPS) for c in range(2)], SR)
    ctx.Destination.SetChannelCount(2)
    for v in range(9):
        s = AudioBufferSourceNode(ctx)
        s.Buffer = PlayableAudioBuffer.FromMonoArray(G.voice(v, 2 * frames + 256), SR)
        g = GainNode(ctx)
        g.Gain.Value = 0.25 + 0.1 * v
        cv = ConvolverNode(ctx)
        cv.Buffer = ir
        s.Connect(g).Connect(cv).Connect(ctx.Destination)
        s.Start()
    return 2


def _config3(voices):
    return lambda ctx, frames: G.config3_convolver(ctx, voices=voices, taps=TAPS, frames=frames)


# name -> (builder(ctx, frames), frames per Render call, Render calls, options)
CASES = {f"v{v}_f{b}": (_config3(v), 128 * b, 1, {}) for v in (9, 65, 130) for b in (3, 259, 260)}
CASES["looping_unaligned"] = (_looping_unaligned, F259, 2, {})
CASES["carry"] = (_behind_gains, F259, 2, {"coarse_tail": 0})


def render_case(name, ctx, wgs_per_cu=None, device=True):
    build, frames, calls, opts = CASES[name]
    if wgs_per_cu is not None:
        ctx.SetOption("coarse_premix_wgs_per_cu", wgs_per_cu)
    if device:
        ctx.SetOption("coarse_min_blocks", 1)
        for k, v in opts.items():
            ctx.SetOption(k, v)
    ch = build(ctx, frames)
    out = np.zeros((ch, frames * calls), np.float32)
    for i in range(calls):
        ctx.Render(out, frames, i * frames)
    return out


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).digest(), np.uint8)


_golden = {}
_oracle = {}


def golden():
    if not _golden:
        with np.load(GOLDEN) as z:
            _golden.update({k: z[k] for k in z.files})
    return _golden


def oracle(name):
    if name not in _oracle:
        o = OracleContext(SR)
        _oracle[name] = render_case(name, o, device=False)
        o.Dispose()
    return _oracle[name]


@pytest.mark.parametrize("name", list(CASES))
def test_bit_for_bit_what_one_workgroup_per_256_frames_rendered(name):
    gold = golden()
    ref = oracle(name)
    assert G.rms(ref) > 1e-5
    for r in (1, 3, 7):
        h = OfflineAudioContext(SR)
        got = render_case(name, h, wgs_per_cu=r)
        st = h.GetStats()
        h.Dispose()
        assert st["coarse_premixed_signals"] > 0 and st["stage_launches"][10] > 0
        assert np.array_equal(got[:, ::8], gold[name + "__every8th"]), (name, r)
        assert np.array_equal(digest(got), gold[name + "__sha256"]), (name, r)
        err = G.rms(ref - got)
        assert err <= 1e-5, (name, r, err)


def test_the_option_takes_1_to_8():
    h = OfflineAudioContext(SR)
    for bad in (0, 9, 2.5):
        with pytest.raises(Exception):
            h.SetOption("coarse_premix_wgs_per_cu", bad)
    h.SetOption("coarse_premix_wgs_per_cu", 8)
    h.Dispose()
