"""The node kernels at production chunk lengths: every scene of tests/_long_scenes.py rendered on the device as ONE chunk of 2200
blocks (default options) or 4200 blocks (`max_chunk_blocks` = 8192), so that the launch shapes of ga_kernels.hip and ga_biquad.hip cross the boundaries
short renders never reach: the serial carry across groups of 64 blocks and their ragged last group, workgroups of 64 blocks from
`bl0`, and the grids capped at 1024, 2048 and 4096 blocks, which stride from there on.

The references are the CPU oracle (array_equal), the double-trig oracle where a kernel evaluates cos / sin / pow (the convention of
tests/test_gpu_param_edges.py), and the numpy models that tests/test_oracle_long_chunks.py pins against the oracle.  Every device
render asserts its chunk count (LS.render): a chunk split by the memory limit fails the test.  Every mismatch prints the first
differing frame with its block, group and stride index (LS.same)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from graphaudio_amd import OfflineAudioContext, OscillatorType
from tests import _graphs as G
from tests import _long_scenes as LS
from tests._oracle import OracleContext

B = LS.B
FRAMES = LS.L1 * B
DEV = OfflineAudioContext


def device(name, opts=None, **kw):
    """(output, stats) of SCENES[name] on the device: one chunk per render call, asserted; the L2 scenes with L2_OPTS."""
    scene = LS.SCENES[name]
    o = dict(LS.L2_OPTS) if scene.frames == LS.L2 * B else {}
    o.update(opts or {})
    return LS.render(DEV, scene, opts=o, **kw)


def within_the_sin_class(ref, got, name):
    """The oscillator bounds of tests/test_gpu_nodes2.py: the device's sin(double) and the C library's differ in the last bit of the
    double now and then, which can move the float by one ulp -- at most 1.2e-7, on fewer than 1 sample in 1000."""
    diff = np.abs(ref.astype(np.float64) - got)
    bad = np.flatnonzero(diff[0])
    where = f", first {bad[0]} = block {bad[0] // B}, group {bad[0] // B // LS.GROUP}" if len(bad) else ""
    print(f"{name}: max |diff| {float(diff.max()):.3e}, {len(bad)} differing frames{where}")
    assert G.rms(ref) > 0.1
    assert diff.max() <= LS.OSC_MAX_ABS
    assert np.mean(ref != got) < LS.OSC_SHARE


# ---- L1: 2200 blocks, default options ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("typ", list(OscillatorType), ids=lambda t: t.name)
def test_oscillator_constant_frequency(typ):
    """Scene 1.  oscillator_kernel: the serial phase carry (`__shfl`) across 35 groups of 64 blocks, the last one ragged (24 blocks)
    with the Stop inside it; in two calls cut inside group 15 the phase travels through job.phase instead."""
    name = f"osc_const_{typ.name}"
    ref = LS.oracle(name)
    got, _ = device(name)
    within_the_sin_class(ref, got, name)
    assert not got[0, :LS.OSC_FIRST].any() and not got[0, LS.OSC_END:].any()
    if typ == OscillatorType.Sine:
        err = float(np.abs(got[0] - LS.sine_closed_form(FRAMES)).max())
        print(f"{name}: device vs closed form {err:.3e}")
        assert err <= LS.SINE_CLOSED_FORM
    two, _ = device(name, pieces=LS.OSC_PIECES)
    LS.same(got, two, name + " one call vs two calls")


def test_oscillator_frequency_curve():
    """Scene 2.  oscillator_kernel with a per-sample frequency from param_curve_kernel, across the groups of 64 blocks and the 1024-
    and 2048-block edges of the curve's grid."""
    curve, _ = device("osc_curve_as_offset")
    LS.same(LS.oracle("osc_curve_as_offset"), curve, "osc_curve: the frequency curve itself")   # the precondition: bit-identical increments
    ref = LS.oracle("osc_curve")
    got, _ = device("osc_curve")
    within_the_sin_class(ref, got, "osc_curve")


@pytest.mark.parametrize("name", ["loop_rate1", "loop_rate1_window"])
def test_looping_source(name):
    """Scene 3.  loop_source_kernel: the grid capped at 1024 x 256 frames strides from block 2048 on."""
    got, _ = device(name)
    LS.same(LS.oracle(name), got, name)
    buf = LS.loop_buffer()
    idx = LS.loop_window_indices(LS.L1) if name.endswith("window") else np.arange(FRAMES) % len(buf)
    LS.same(buf[idx], got[0], name + " against the index model")


@pytest.mark.parametrize("fast", [1, 0])
@pytest.mark.parametrize("name", ["resample_noloop", "resample_ends"])
def test_resampled_source(name, fast):
    """Scene 4.  resample_fast_kernel: 512 workgroups x 256 samples, then strides (from block 1024 on); resample_kernel (option
    resample_fast = 0): 35 workgroups of 64 blocks per job, the last one ragged.  resample_ends: the buffer runs out inside block 2100."""
    ref = LS.oracle(name)
    got, _ = device(name, opts={"resample_fast": fast})
    LS.same(ref, got, f"{name} resample_fast={fast}")
    assert G.rms(ref) > 0.1
    if name == "resample_noloop":
        err = float(np.abs(got[0] - LS.resample_model(LS.resample_buffer(), FRAMES)).max())
        print(f"{name}: device vs float64 model {err:.3e}")
        assert err <= 4 * LS.RESAMPLE_MODEL_ERR
    else:
        assert not got[0, LS.RESAMPLE_END_FRAME + 4:].any() and got[0, LS.RESAMPLE_END_FRAME - 8:LS.RESAMPLE_END_FRAME - 4].any()


def test_looping_resampled_source():
    """Scene 5.  gsr_kernel: 64 blocks per workgroup from `bl0`, 35 workgroups, the last one ragged (early return before the barrier)."""
    ref = LS.oracle("gsr_loop")
    got, _ = device("gsr_loop")
    assert G.rms(ref) > 0.1
    LS.same(ref, got, "gsr_loop")


def test_constant_delay():
    """Scene 6.  delay_kernel: the grid capped at 1024 x 256 frames strides from block 2048 on."""
    got, _ = device("delay_const")
    LS.same(LS.oracle("delay_const"), got, "delay_const")
    x = G.voice(74, FRAMES)
    assert not got[0, :LS.DELAY_FRAMES].any()
    LS.same(x[:FRAMES - LS.DELAY_FRAMES], got[0, LS.DELAY_FRAMES:], "delay_const against the shifted input")


def test_moving_delay():
    """Scene 7.  delay_kernel with a delay time per sample (param_curve_kernel), two channels, past 2048 blocks."""
    ref = LS.oracle("delay_ramp")
    got, _ = device("delay_ramp")
    assert G.rms(ref[0]) > 1e-2 and G.rms(ref[1]) > 1e-2
    LS.same(ref, got, "delay_ramp")


def test_delay_onset_scan_past_1024_blocks():
    """Scene 8.  delay_onset_kernel: 256 workgroups x 4 waves, then strides, `break` on the first hit: the onset is in block 1179."""
    ref = LS.oracle("delay_onset")
    got, st = device("delay_onset", opts={"delay_flag_exact": 1})
    assert st["delay_flags_read"] > 0
    assert G.rms(ref[:, LS.ONSET_WINDOW] - LS.oracle("delay_onset_control")[:, LS.ONSET_WINDOW]) >= 1e-3   # (the scene tells an early flag)
    LS.same(ref, got, "delay_onset")


@pytest.mark.parametrize("law", ["stereo", "mono"])
def test_automated_panner(law):
    """Scene 9.  stereo_panner_dynamic_kernel: {last pan, gains} through `carry[nb]` across 35 groups of 64 blocks, the last one ragged;
    changes in blocks 1023 / 1024, 2047 / 2048, 2175 and at the first frame of the ragged group."""
    name = f"pan_long_{law}"
    ref = LS.dtrig(name)
    assert np.isfinite(ref).all() and G.rms(ref) > 1e-3
    got, _ = device(name)
    LS.same(ref, got, name)


@pytest.mark.parametrize("kind", ["held", "returned"])
def test_panner_state_carried_through_every_group(kind):
    """Scene 9, the carried state.  stereo_panner_dynamic_kernel: gains that are no function of the pan (block 0's stereo-law gains on
    a mono source; the mono law's at the same pan) handed from group to group of 64 blocks through `carry[nb]`, 33 times, with no change
    of the pan that would recompute them (tests/test_oracle_long_chunks.py proves on the oracle which blocks depend on it)."""
    name = f"pan_carried_{kind}"
    ref = LS.dtrig(name)
    assert np.isfinite(ref).all() and G.rms(ref) > 1e-3
    got, _ = device(name)
    LS.same(ref, got, name)
    LS.same(LS.oracle(name), got, name + " against the plain oracle")


def test_automated_biquad():
    """Scene 10.  biquad_dynamic_kernel: an update at every one of 281,600 samples, two channels, one chunk."""
    ref = LS.dtrig("bq_long")
    assert np.isfinite(ref).all() and np.abs(ref).max() < 10.0 and G.rms(ref) > 1e-3
    got, _ = device("bq_long")
    LS.same(ref, got, "bq_long")


def test_gain_curve_and_audio_rate_modulation():
    """Scene 11.  gain_kernel with `curve` and `mod`, param_mod_kernel a-rate: grids capped at 1024 x 256 frames."""
    ref = LS.oracle("gain_mod")
    assert G.rms(ref[0]) > 1e-2 and G.rms(ref[1]) > 1e-2 and len(np.unique(ref[1])) > 1000
    got, _ = device("gain_mod")
    LS.same(ref, got, "gain_mod")


def test_k_rate_modulation():
    """Scene 11, k-rate.  param_mod_kernel with `krate` past 2048 blocks, read by biquad_dynamic_kernel."""
    ref = LS.dtrig("krate_mod")
    assert np.isfinite(ref).all() and np.abs(ref).max() < 10.0 and G.rms(ref) > 1e-3
    got, _ = device("krate_mod")
    LS.same(ref, got, "krate_mod")


def strided_timeline_check(row, tl, blocks, first=0, end=None):
    frames = np.arange(0, blocks * B, LS.STRIDE)
    want = LS.timeline_at(tl, frames, blocks)
    want[(frames < first) | (frames >= (blocks * B if end is None else end))] = 0.0
    LS.same(want, row[frames], "every 97th frame against the timeline's restatement")


def test_constant_source_window():
    """Scene 12.  const_source_kernel and param_curve_kernel: 1024 x 256 frames, then strides; Stop inside block 2100."""
    got, _ = device("const_window")
    LS.same(LS.oracle("const_window"), got, "const_window")
    first, end = LS.window_frames(LS.CONST_START, LS.CONST_STOP, LS.L1)
    strided_timeline_check(got[0], LS.const_timeline(), LS.L1, first, end)


def test_stream_source():
    """Scene 13.  stream_kernel: 64 blocks per workgroup from `bl0`, 35 workgroups, the last one ragged; six 44.1 kHz buffers."""
    from tests.test_stream_source import _buffers
    scene = LS.stream_long(_buffers)
    def queue(hold):
        return hold[0].QueuedBufferCount, hold[0].ProcessedBufferCount
    ref, _, ref_queue = LS.render(OracleContext, scene, probe=queue)
    got, _, got_queue = LS.render(DEV, scene, probe=queue)
    assert G.rms(ref) > 1e-3 and G.rms(ref[:, 2100 * B:]) > 1e-3
    LS.same(ref, got, "stream_long")
    assert ref_queue == got_queue and ref_queue[1] >= 4, (ref_queue, got_queue)   # buffers retired inside the chunk


def test_spatial_panner_whole_against_chunked():
    """Scene 14.  spatial_panner_kernel / spatial_desc_kernel: the ramp scene of tests/test_gpu_spatial.py stretched to 2200 blocks,
    one chunk against chunks of 4 blocks."""
    from tests import _spatial_model as M
    from tests.test_gpu_spatial import moving_scene, noise_set
    h = noise_set(8 * 3, 129, 77)
    x = G.voice(31, FRAMES)
    bt = M.block_times(LS.L1, LS.SR)
    scene = LS.Scene("spatial_long", lambda ctx: moving_scene(ctx, x, h, 8, "ramp", bt), LS.L1, ch=2)
    whole, _ = LS.render(DEV, scene)
    chunked, _ = LS.render(DEV, scene, opts={"max_chunk_blocks": 4}, chunks=LS.L1 // 4)
    assert G.rms(whole) > 1e-3 and G.rms(whole[:, 2100 * B:]) > 1e-4
    LS.same(whole, chunked, "spatial_long whole vs chunks of 4")


# ---- L2: 4200 blocks, max_chunk_blocks = 8192 ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("voices", [330, 40])
def test_bus(voices):
    """Scene 15.  330 terms: mix_wide_kernel, 8192 workgroups x 64 frames, then strides (from frame 524,288 on), ragged last batch of
    10 terms.  40 terms, one view a frame off alignment: mix_kernel<1, true>, 2048 x 256 frames, the same edge."""
    name = f"bus_{voices}"
    ref = LS.oracle(name)
    assert G.rms(ref) > 1e-2 and G.rms(ref[:, 4096 * B:]) > 1e-2
    got, _ = device(name)
    LS.same(ref, got, name)


def test_downmix():
    """Scene 16.  downmix_kernel: 2048 x 256 frames, then strides."""
    ref = LS.oracle("downmix_long")
    assert G.rms(ref) > 1e-2 and G.rms(ref[:, 4096 * B:]) > 1e-2
    got, _ = device("downmix_long")
    LS.same(ref, got, "downmix_long")


def test_parameter_curves_past_4096_blocks():
    """Scene 17.  param_curve_kernel strides past 4096 blocks: a-rate (ConstantSourceNode.offset, GainNode.gain) and k-rate (a
    biquad's gain in dB), events in blocks 4090 .. 4150."""
    ref = LS.dtrig("param_late")
    got, _ = device("param_late")
    LS.same(LS.oracle("param_late")[:2], got[:2], "param_late a-rate")
    LS.same(ref, got, "param_late")
    assert G.rms(ref[2, 4096 * B:]) > 1e-3
    for row in (got[0], got[1]):
        strided_timeline_check(row, LS.const_timeline(True), LS.L2)


@pytest.mark.parametrize("channels", [2, 3])
def test_interleaved_output(channels):
    """Scene 18.  interleave_kernel: 4096 x 256 elements, then strides: 1,075,200 and 1,612,800 elements.  The third channel is
    unused and zero."""
    scene = LS.SCENES["bus_40"]
    planar, _ = LS.render(DEV, scene, opts=LS.L2_OPTS)
    inter = LS.render_interleaved(DEV, scene, channels, opts=LS.L2_OPTS)
    assert G.rms(planar) > 1e-2
    LS.same(planar, inter[:2], f"interleaved, {channels} channels")
    if channels == 3:
        assert not inter[2].any()
