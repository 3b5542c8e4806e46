"""Constant-coefficient BiQuadFilterNode cascades of every length and wave packing, against the CPU oracle.

The oracle restates BiQuadFilterNode.cs:137-138 per sample (tests/test_oracle_graph.py holds its single section to
scipy.signal.lfilter in float64); the one-walk evaluation on the device is the same float arithmetic operation by operation, so the
condition is np.array_equal.  Only the time split (case 6) rounds differently and is measured instead.

Launch rules the cases are derived from (ga_biquad.hip; a change there has to be restated here):

  cascades of 2..8 sections -> biquad_pipe_kernel<NSEC>                                 launch_biquad, `if (pipe && nsec >= 2)`
      GPR  = 16 // NSEC                 cascades per 16-lane row                       biquad_pipe_kernel, `constexpr int GPR`
      MAXJ = min(16, 4 GPR)             cascades per wave at most                      biquad_pipe_kernel, `constexpr int MAXJ`
      jpw  = min(MAXJ, ceil(njobs / 512))                                              launch_biquad_pipe, `int jpw = ...`
      NSEC: GPR / MAXJ =  2: 8/16  3: 5/16  4: 4/16  5: 3/12  6: 2/8  7: 2/8  8: 2/8
      D = 4 (NSEC - 1) steps of pipeline delay, tiles of PT = 256 steps                biquad_pipe_kernel, `constexpr int D`, `PT`
  cascades of 1 section -> biquad_kernel<1, JPW>                                        launch_biquad, `int per = (njobs + 511) / 512`
      JPW = 4 / 8 / 16 / 32 / 64 for njobs <= 2,048 / 4,096 / 8,192 / 16,384 / above
      tiles of 256 frames for JPW <= 8, else 64                                        biquad_kernel, `constexpr int TL`
  a kernel sees whole blocks, n = 128 m per segment of a chunk; one launch per (level, cascade length)   Exec::flushLevel
  chains fuse up to kMaxBiquadSections = 8 nodes (ga_kernels.hpp); a second consumer, an automated node or a change of the
  channel count ends a chain                                                            Context::chunkPlanNodes, "biquad cascade fusion"
  segments of >= biquad_split_min_frames are cut along time: biquad1_kernel / biquad_kernel<NSEC, 32> (state only, then with
  output) and biquad_scan_fixed_kernel<1..4> / biquad_scan_kernel                       Context::planBiquad, launch_biquad_lanes / _scan

The job count of a launch is reached through the graph alone: a biquad node yields one job per channel, so a 32-channel source (the
maximum, tests/test_gpu_edges.py) with 32 different channels through a chain of k nodes is 32 cascades of k sections; 241 such
chains are 7,712 cascades.  The sources share eight 32-channel buffers (different filter settings on the same buffer give
different outputs), so host memory stays small.  Every case renders in several calls: the lengths vary, and every call after the
first starts from the state the previous one left in device memory.

Filters are well-conditioned mid-band sections throughout (peaking or low-pass, 1-14 kHz, Q <= 1.5, gains within +/-6 dB), varied per
chain and per section.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from graphaudio_amd import (AudioBufferSourceNode, BiQuadFilterNode, ChannelCountMode, FilterType, OfflineAudioContext,
                            PlayableAudioBuffer)
from tests import _graphs as G
from tests._oracle import DtrigOracleContext, OracleContext
from tests._report import note

SR = 48000
B = 128
NBUF = 8          # shared 32-channel sample buffers
MAXCH = 32


def gpr(k):
    return 16 // k


def maxj(k):
    return min(16, 4 * gpr(k))


def jpw_of(k, njobs):
    return min(maxj(k), max(1, -(-njobs // 512)))


def jpw1_of(njobs):
    per = -(-njobs // 512)
    return 4 if per <= 4 else 8 if per <= 8 else 16 if per <= 16 else 32 if per <= 32 else 64


assert [(gpr(k), maxj(k)) for k in range(2, 9)] == [(8, 16), (5, 16), (4, 16), (3, 12), (2, 8), (2, 8), (2, 8)]

_ROWS = {}


def rows(b, frames):
    """channel arrays of shared buffer b, cut to `frames` (generated once, at the longest length any case asks for)"""
    full = 128 * 96
    assert frames <= full
    if b not in _ROWS:
        _ROWS[b] = [G.voice(7000 + 100 * b + c, full) for c in range(MAXCH)]
    return [r[:frames] for r in _ROWS[b]]


def sections(chain, k, mild=False):
    """k mid-band sections (type, frequency, Q, gain dB) for chain number `chain`; mild: 3-14 kHz, Q <= 1, within +/-4 dB -- cascades
    whose predicted rounding deviation (Context::biquadDeviation) is so far below option biquad_split_max_deviation that mode 1 of
    the time split takes every one of them"""
    rng = np.random.default_rng(90000 + 17 * chain + 1009 * k)
    out = []
    for q in range(k):
        f = float(3000.0 * (14.0 / 3.0) ** rng.random()) if mild else float(1000.0 * 14.0 ** rng.random())
        qq = float(0.5 + (0.5 if mild else 1.0) * rng.random())
        if rng.random() < 0.7:
            gain = float(rng.uniform(1.5, 4.0 if mild else 6.0)) * (1 if (q + chain) % 2 else -1)    # alternating: the cascade stays near unity
            out.append((FilterType.Peaking, f, qq, gain))
        else:
            out.append((FilterType.Lowpass, max(f, 3000.0), qq, 0.0))
    for (_, f, qq, g) in out:
        assert 1000.0 <= f <= 14000.0 and qq <= 1.5 and abs(g) <= 6.0
    return out


def biquad(ctx, spec):
    ft, f, q, g = spec
    bq = BiQuadFilterNode(ctx)
    bq.Type = ft
    bq.Frequency.Value = f
    bq.Q.Value = q
    bq.Gain.Value = g
    return bq


class Chain:
    """one source (channels `ch` of shared buffer `buf`) through k biquads into the destination"""

    def __init__(self, index, k, ch=MAXCH, when=0.0, offset=0, length=None):
        self.index, self.k, self.ch, self.when, self.offset, self.length = index, k, ch, when, offset, length
        self.secs = sections(index, k)


def add_chain(ctx, bufs, c, frames, into=None):
    key = (c.index % NBUF, c.ch, c.length)
    if key not in bufs:
        bufs[key] = PlayableAudioBuffer.FromChannelArrays(rows(key[0], c.length or frames)[:c.ch], SR)
    s = AudioBufferSourceNode(ctx)
    s.Buffer = bufs[key]
    node = s
    nodes = []
    for spec in c.secs:
        node = node.Connect(biquad(ctx, spec))
        nodes.append(node)
    node.Connect(into or ctx.Destination)
    s.Start(c.when, (c.offset + 0.5) / SR if c.offset else 0.0)   # (int64)(offset * sampleRate): + 0.5 keeps the truncation off an edge
    return nodes


def graph_of(chains, dest_ch, total):
    """builder: the chains into a destination of dest_ch channels; sample buffers last beyond the render (no source ends)"""
    def build(ctx):
        ctx.Destination.SetChannelCount(dest_ch)
        bufs = {}
        for c in chains:
            add_chain(ctx, bufs, c, total + 2 * B + 4)
        return dest_ch
    return build


def render(mk, build, pieces, **opts):
    ctx = mk(SR)
    for k, v in opts.items():
        ctx.SetOption(k, v)
    ch = build(ctx)
    out = np.zeros((ch, sum(pieces)), np.float32)
    pos = 0
    for n in pieces:
        ctx.Render(out, n, pos)
        pos += n
    st = ctx.GetStats() if mk is OfflineAudioContext else None
    ctx.Dispose()
    return out, st


def same_bits(ref, got, what):
    assert np.isfinite(ref).all() and G.rms(ref) > 1e-3, what
    if np.array_equal(ref, got):
        return
    bad = ref != got
    rws = np.flatnonzero(bad.any(axis=1))
    frs = np.flatnonzero(bad.any(axis=0))
    raise AssertionError(f"{what}: {int(bad.sum())} samples differ, rows {rws[:8].tolist()} ({len(rws)} of {ref.shape[0]}), "
                         f"frames {frs[:8].tolist()} .. {int(frs[-1])}, max abs {float(np.abs(ref - got).max()):.3e}")


def packed_chains(k, njobs_lo, njobs_hi, jpw):
    """32-channel chains plus one of fewer channels (5, or 7 where 5 would fill the last wave): njobs_lo + 32 + 5 cascades
    (njobs_lo is a multiple of 32), `jpw` of them per wave and the last wave partial"""
    full = njobs_lo // MAXCH + 1
    short = next(c for c in (5, 7) if (MAXCH * full + c) % jpw)
    chains = [Chain(i, k) for i in range(full)] + [Chain(full, k, ch=short)]
    njobs = sum(c.ch for c in chains)
    assert njobs_lo < njobs <= njobs_hi and njobs % jpw != 0, (k, njobs, njobs_lo, njobs_hi, jpw)
    assert (jpw1_of(njobs) if k == 1 else jpw_of(k, njobs)) == jpw, (k, njobs, jpw)
    return chains, njobs


# ---- 1. every length, one cascade per wave, nothing summed ------------------------------------------------------------------
PIECES_1 = [B, 2 * B, 3 * B, 5 * B, 2 * B, 9 * B]


@pytest.mark.parametrize("k", range(1, 9))
def test_every_length_one_cascade_per_wave_every_cascade_its_own_row(k):
    """n below / at / above a 256-step tile, n + D on both sides of a tile edge (n = 256: the second tile is all drain), three-tile
    walks whose middle tile takes the whole-tile 16-byte path (n = 640, 1152); 32 cascades, each on its own output row"""
    build = graph_of([Chain(k, k)], MAXCH, sum(PIECES_1))
    assert jpw_of(k, MAXCH) == 1 and jpw1_of(MAXCH) == 4
    ref, _ = render(OracleContext, build, PIECES_1)
    assert min(G.rms(r) for r in ref) > 1e-4      # every row carries its cascade
    got, _ = render(OfflineAudioContext, build, PIECES_1)
    same_bits(ref, got, f"{k} sections")


# ---- 2. wave packing ------------------------------------------------------------------------------------------------------
PIECES_2 = [B, 3 * B, 5 * B]


def _packings():
    out = []
    for k in range(2, 9):
        for j in sorted({2, gpr(k) + 1, maxj(k)}):
            if j <= maxj(k):
                out.append((k, j))
    return out


@pytest.mark.parametrize("k,jpw", _packings(), ids=lambda v: str(v))
def test_wave_packing_pipelined(k, jpw):
    """jpw = 2 (second slot of the first lane row), GPR + 1 (first slot of the second row), MAXJ (all rows); njobs % jpw != 0: the
    last wave is partial"""
    chains, njobs = packed_chains(k, 512 * (jpw - 1), 512 * jpw, jpw)
    build = graph_of(chains, MAXCH, sum(PIECES_2))
    ref, _ = render(OracleContext, build, PIECES_2)
    got, _ = render(OfflineAudioContext, build, PIECES_2)
    same_bits(ref, got, f"{k} sections, {njobs} cascades, {jpw} per wave")


@pytest.mark.parametrize("jpw,lo,hi", [(8, 2048, 4096), (16, 4096, 8192), (32, 8192, 16384), (64, 16384, 1 << 20)])
def test_wave_packing_single_section(jpw, lo, hi):
    """biquad_kernel<1, 8 / 16 / 32 / 64>: the recursive half per lane, the FIR half over the tile (prevw), tiles of 256 and 64"""
    chains, njobs = packed_chains(1, lo, hi, jpw)
    build = graph_of(chains, MAXCH, sum(PIECES_2))
    ref, _ = render(OracleContext, build, PIECES_2)
    got, _ = render(OfflineAudioContext, build, PIECES_2)
    same_bits(ref, got, f"1 section, {njobs} cascades, {jpw} per wave")


# ---- 3. rows that are not 16-byte aligned -------------------------------------------------------------------------------------
PIECES_3 = [6 * B, 7 * B, 6 * B]


@pytest.mark.parametrize("packed", [False, True], ids=["35", "packed"])
@pytest.mark.parametrize("k", [1, 2, 5, 8])
def test_rows_off_16_bytes_and_late_starts(k, packed):
    """sources read their buffers from sample 1, 2 or 3 (zero-copy: the cascade's input row IS the buffer window), others start in
    blocks 1, 3 and 8 at times inside the block: several segments per call, up to six blocks long (three tiles: the whole-tile
    16-byte loads of the pipelined kernel run on rows that are 4, 8 and 12 bytes off)"""
    if packed:
        chains, njobs = packed_chains(k, 2048, 4096, 8) if k == 1 else packed_chains(k, 512, 1024, 2)
    else:
        chains = [Chain(i, k, ch=4) for i in range(8)] + [Chain(8, k, ch=3)]
        njobs = 35
    assert sum(c.ch for c in chains) == njobs
    for i, c in enumerate(chains):
        c.offset = (i // 2) % 4
        if i % 2:
            c.when = (B * (1, 3, 8)[(i // 2) % 3] + 37.25) / SR
    assert {c.offset for c in chains if c.when == 0.0} == {0, 1, 2, 3} == {c.offset for c in chains if c.when > 0.0}
    build = graph_of(chains, MAXCH, sum(PIECES_3))
    ref, _ = render(OracleContext, build, PIECES_3)
    got, st = render(OfflineAudioContext, build, PIECES_3)
    assert st["segments"] >= 6     # per call: blocks 0 | 1-2 | 3-5, 6-7 | 8-12, 13-18
    same_bits(ref, got, f"{k} sections, {njobs} cascades, offsets and late starts")


# ---- 4. the fusion cap and broken chains -----------------------------------------------------------------------------------------
PIECES_4 = [3 * B, B, 5 * B, 3 * B]


def _cap(ctx):           # 9, 16, 17 nodes: 8 + 1, 8 + 8, 8 + 8 + 1
    return graph_of([Chain(40 + n, n, ch=5) for n in (9, 16, 17)], 5, sum(PIECES_4))(ctx)


def _tap(ctx):           # the third of six nodes also feeds the destination: absorption stops there, 3 + 3
    ctx.Destination.SetChannelCount(5)
    nodes = add_chain(ctx, {}, Chain(50, 6, ch=5), sum(PIECES_4) + 2 * B)
    nodes[2].Connect(ctx.Destination)
    return 5


def _timeline(ctx):      # the third of five nodes has its frequency on a timeline: 2 constant + biquad_dynamic_kernel + 2 constant
    ctx.Destination.SetChannelCount(5)
    nodes = add_chain(ctx, {}, Chain(60, 5, ch=5), sum(PIECES_4) + 2 * B)
    # steps (bit-equal between the plain and the double-trig oracle: DESIGN.md section 8, "libm class"; asserted below)
    for i, f in enumerate((2000.0, 3500.0, 1000.0, 5000.0)):
        nodes[2].Frequency.SetValueAtTime(f, (2.5 * i * B + 40) / SR)
    return 5


def _mono_to_stereo(ctx):   # two explicit-mono nodes, then two explicit-stereo nodes (twin channels): 2 + 2
    ctx.Destination.SetChannelCount(2)
    nodes = add_chain(ctx, {}, Chain(70, 4, ch=2), sum(PIECES_4) + 2 * B)
    for i, n in enumerate(nodes):
        n.Inputs[0].SetChannelCount(1 if i < 2 else 2)
        n.Inputs[0].SetChannelCountMode(ChannelCountMode.Explicit)
    return 2


def _all_lengths(ctx):   # chains of 1..8 nodes side by side: their last nodes sit in different levels, one launch per length
    return graph_of([Chain(80 + k, k) for k in range(1, 9)], MAXCH, sum(PIECES_4))(ctx)


def _all_lengths_one_level(ctx):   # chains of 8 nodes tapped after node 8 - k: cascades of 8 - k and of k sections, and the
    # cascades of k = 1..8 sections all END eight nodes behind a source -- in one level, one launch per length
    ctx.Destination.SetChannelCount(6)
    bufs = {}
    for k in range(1, 9):
        nodes = add_chain(ctx, bufs, Chain(90 + k, 8, ch=6), sum(PIECES_4) + 2 * B)
        if k < 8:
            nodes[7 - k].Connect(ctx.Destination)
    return 6


@pytest.mark.parametrize("build", [_cap, _tap, _timeline, _mono_to_stereo, _all_lengths, _all_lengths_one_level],
                         ids=lambda f: f.__name__.strip("_"))
def test_fusion_cap_and_broken_chains(build):
    ref, _ = render(OracleContext, build, PIECES_4)
    if build is _timeline:
        dtrig, _ = render(DtrigOracleContext, build, PIECES_4)
        assert np.array_equal(ref, dtrig)     # the automated node's coefficients do not depend on the libm here: one reference
        one, _ = render(OracleContext, build, [sum(PIECES_4)])
        assert np.array_equal(ref, one)
    got, _ = render(OfflineAudioContext, build, PIECES_4)
    same_bits(ref, got, build.__name__)


# ---- 5. falling silent and resuming -------------------------------------------------------------------------------------------
PIECES_5 = [4 * B, 6 * B, 6 * B]
ENDS = (2, 3, 4, 5)          # block after which the first source of chain i is over
RESUMES = (8, 9, 10, 11)     # block in which its second source starts


def _silence(ctx):
    ctx.Destination.SetChannelCount(3)
    for i, (e, r) in enumerate(zip(ENDS, RESUMES)):
        c = Chain(100 + i, 3 if i % 2 == 0 else 6, ch=3, length=B * e + 1)   # e whole blocks; the block that would end the buffer is dropped
        nodes = add_chain(ctx, {}, c, 0)
        s2 = AudioBufferSourceNode(ctx)
        s2.Buffer = PlayableAudioBuffer.FromChannelArrays(rows((i + 4) % NBUF, sum(PIECES_5) + 2 * B)[:3], SR)
        s2.Connect(nodes[0])
        s2.Start((B * r + 64.5) / SR)
    return 3


def test_cascades_fall_silent_and_resume():
    """the reference freezes a biquad's state while its input is silent and clears its output (BiQuadFilterNode.cs:103-108;
    tests/test_oracle_graph.py::test_biquad_silent_input_freezes_state): chains of 3 and 6 sections whose sources end at blocks
    2..5 and whose second sources start at blocks 8..11 -- the launches' job count changes from segment to segment, a cascade
    resumes from the state it froze"""
    ref, _ = render(OracleContext, _silence, PIECES_5)
    assert not ref[:, B * max(ENDS):B * min(RESUMES)].any()                          # exact silence between the sources
    assert all(G.rms(ref[:, B * b:B * (b + 1)]) > 1e-3 for b in range(0, min(ENDS)))
    assert all(G.rms(ref[:, B * b:B * (b + 1)]) > 1e-3 for b in range(min(RESUMES), 16))   # ... and sound after the resume
    got, st = render(OfflineAudioContext, _silence, PIECES_5)
    assert st["segments"] >= 8     # blocks 0-1 | 2 | 3, 4 | 5-7 | 8 | 9, 10 | 11-15
    same_bits(ref, got, "silence and resume")


# ---- 6. the time split, by cascade length ---------------------------------------------------------------------------------------
PIECES_6 = [17 * B, 25 * B, 10 * B, 41 * B]    # two pieces | three, the last one shorter | below the threshold: one walk | five pieces


def _split_graph(k):
    def build(ctx):
        ctx.Destination.SetChannelCount(2)
        total = sum(PIECES_6) + 2 * B
        for v in range(6):
            secs = sections(200 + v, k, mild=True)
            s = AudioBufferSourceNode(ctx)
            if v < 5:   # a stereo source with two different channels: two cascades
                s.Buffer = PlayableAudioBuffer.FromChannelArrays(rows(v % NBUF, total)[2 * v:2 * v + 2], SR)
            else:       # mono material in stereo nodes: twin channels, one cascade evaluated for both
                s.Buffer = PlayableAudioBuffer.FromMonoArray(rows(v % NBUF, total)[20], SR)
            node = s
            for spec in secs:
                bq = biquad(ctx, spec)
                if v == 5:
                    bq.Inputs[0].SetChannelCount(2)
                    bq.Inputs[0].SetChannelCountMode(ChannelCountMode.Explicit)
                node = node.Connect(bq)
            node.Connect(ctx.Destination)
            s.Start()
        return 2
    return build


SPLIT_CASCADES = 3 * (5 * 2 + 1)   # the three calls of >= 2048 frames, one chunk and one segment each: 10 stereo rows + 1 twin pair


@pytest.mark.parametrize("k", range(1, 9))
def test_time_split_by_cascade_length(k):
    """biquad1_kernel<true / false> (k = 1), state-only and full biquad_kernel<k, 32>, biquad_scan_fixed_kernel<1..4> and the generic
    scan (5..8), default mode 1 with the threshold lowered to 2048 frames.  Without the split the pieces are bit-equal to the oracle;
    with it every output channel stays within 2e-6 relative and 1e-5 absolute RMS (tests/test_gpu_biquad_split.py for this filter
    family; the north-star contract): a hand-over or scan error is O(1e-2..1).
    Measured on MI355X: 0 for every k -- these sections are damped so strongly (pole radius <= 0.9) that a piece's start state no
    longer reaches its end state, not even through the rounding sequence, so a piece handed the right state reproduces the one walk;
    with the wider family of the other cases (1 kHz, Q 1.5) the same graph measures 2e-8 .. 2e-7, and mode 1 declines two of its
    cascades.  What A^K carries across a piece is tests/test_gpu_biquad_split.py's subject (low cut-offs)."""
    build = _split_graph(k)
    ref, _ = render(OracleContext, build, PIECES_6)
    one, st1 = render(OfflineAudioContext, build, PIECES_6, biquad_time_split=0, biquad_split_min_frames=2048)
    assert st1["biquad_split_cascades"] == 0
    same_bits(ref, one, f"{k} sections, one walk")
    got, st = render(OfflineAudioContext, build, PIECES_6, biquad_split_min_frames=2048)
    errs = [(G.rms(ref[c] - got[c]), G.rms(ref[c])) for c in range(2)]
    note(f"[biquad cascades] time split, {k} sections: {st['biquad_split_cascades']} cascades split; per channel rms "
         + ", ".join(f"{s:.4f}" for _, s in errs) + "; vs oracle abs " + ", ".join(f"{e:.3e}" for e, _ in errs)
         + "; relative " + ", ".join(f"{e / s:.3e}" for e, s in errs))
    assert st["biquad_split_cascades"] == SPLIT_CASCADES
    assert st["twin_rows"] > 0
    for e, s in errs:
        assert e <= 2e-6 * s and e <= 1e-5, (k, e, s)
