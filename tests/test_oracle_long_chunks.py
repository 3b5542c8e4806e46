"""The references of tests/test_gpu_long_chunks.py, pinned without a GPU: the numpy models of tests/_long_scenes.py against the CPU
oracle at L1 = 2200 blocks, and the relation between the plain and the double-trig oracle that the GPU file assumes scene by scene."""
import numpy as np
import pytest

from graphaudio_amd import OscillatorType
from tests import _graphs as G
from tests import _long_scenes as LS
from tests._oracle import OracleContext

B = LS.B
FRAMES = LS.L1 * B


def test_lengths_cross_the_launch_shapes():
    assert LS.L1 == 34 * 64 + 24 and LS.L1 > 2048 and LS.L2 > 4096 and LS.L2 * B > 524288 and LS.L2 <= LS.L2_OPTS["max_chunk_blocks"]
    assert LS.OSC_PIECES[0] // B % 64 != 0 and sum(LS.OSC_PIECES) == FRAMES
    assert LS.OSC_END // B >= 34 * 64                         # the oscillator stops inside the ragged group
    assert LS.ONSET_ZEROS // B > 1024                         # the onset scan passes the first 1024 blocks
    assert (LS.L1 * B * LS.RATE) / B > 1024                   # (and so does the resampler's input)


# ---- scene 1: oscillator ---------------------------------------------------------------------------------------------------------

def test_sine_closed_form():
    """sin(2 pi 997 (n - 301) / sr): the oracle's phase accumulator (double, wrapped at 2 pi) stays within half a float ulp of it over
    281,600 samples."""
    ref = LS.oracle("osc_const_Sine")[0]
    want = LS.sine_closed_form(FRAMES)
    err = float(np.abs(ref - want).max())
    print(f"oracle sine vs closed form: max error {err:.3e}")
    assert G.rms(ref) > 0.5
    assert not ref[:LS.OSC_FIRST].any() and ref[LS.OSC_FIRST + 1] != 0 and not ref[LS.OSC_END:].any() and ref[LS.OSC_END - 1] != 0
    assert err <= LS.SINE_CLOSED_FORM


@pytest.mark.parametrize("typ", [OscillatorType.Square, OscillatorType.Sawtooth, OscillatorType.Triangle], ids=lambda t: t.name)
def test_oscillator_window(typ):
    ref = LS.oracle(f"osc_const_{typ.name}")[0]
    assert LS.window_frames(300.2 / LS.SR, (LS.OSC_END + 0.5) / LS.SR, LS.L1) == (LS.OSC_FIRST, LS.OSC_END)
    assert not ref[:LS.OSC_FIRST].any() and not ref[LS.OSC_END:].any() and G.rms(ref[LS.OSC_FIRST:LS.OSC_END]) > 0.5
    period = LS.SR / 997.0     # every period of the wave is there: no stretch of a period's length is constant or silent
    live = ref[LS.OSC_FIRST:LS.OSC_END]
    changes = np.flatnonzero(live[1:] != live[:-1])
    assert np.diff(changes).max() <= period


# ---- scene 3: looping rate-1 source ------------------------------------------------------------------------------------------------

def test_loop_rate1_model():
    buf = LS.loop_buffer()
    assert np.array_equal(LS.oracle("loop_rate1")[0], buf[np.arange(FRAMES) % len(buf)])


def test_loop_window_model():
    buf = LS.loop_buffer()
    idx = LS.loop_window_indices(LS.L1)
    assert idx.min() == LS.LOOP_START and idx.max() == LS.LOOP_END - 1 and idx[0] == LS.LOOP_START and idx[B] != LS.LOOP_START + B
    assert np.array_equal(LS.oracle("loop_rate1_window")[0], buf[idx])


# ---- scene 4: resampled source -----------------------------------------------------------------------------------------------------

def test_resampler_model():
    """The measurement behind LS.RESAMPLE_MODEL_ERR: max |oracle - float64 model| over all 281,600 frames of the scene."""
    ref = LS.oracle("resample_noloop")[0]
    want = LS.resample_model(LS.resample_buffer(), FRAMES)
    err = float(np.abs(ref - want).max())
    print(f"oracle resampler vs float64 model: max error {err:.3e} (peak {float(np.abs(want).max()):.3f})")
    assert G.rms(ref) > 0.1
    assert err <= LS.RESAMPLE_MODEL_ERR
    # the bound is the float32 rounding of a polynomial of values below 2: a few ulp of 1, not a tolerance that hides a wrong sample
    assert LS.RESAMPLE_MODEL_ERR <= 16 * np.finfo(np.float32).eps


def test_resampled_buffer_ends_inside_a_block():
    """On the oracle: the partial block (a head of samples, then zeros), silence behind it, the model up to the last sample."""
    ref = LS.oracle("resample_ends")[0]
    b = LS.RESAMPLE_END_FRAME // B
    last = int(np.flatnonzero(ref)[-1])
    assert last // B == b and 0 < last % B < B - 1 and not ref[last + 1:].any()
    assert abs(last - LS.RESAMPLE_END_FRAME) <= 4
    want = LS.resample_model(LS.resample_buffer(True), last + 1)
    assert np.abs(ref[:last + 1] - want).max() <= LS.RESAMPLE_MODEL_ERR


# ---- scene 6: constant delay -------------------------------------------------------------------------------------------------------

def test_constant_delay_is_a_pure_shift():
    ref = LS.oracle("delay_const")[0]
    x = G.voice(74, FRAMES)
    assert int(np.float32(0.3) * np.float32(LS.SR)) == LS.DELAY_FRAMES
    assert not ref[:LS.DELAY_FRAMES].any() and np.array_equal(ref[LS.DELAY_FRAMES:], x[:FRAMES - LS.DELAY_FRAMES])


# ---- scene 12: constant source window ----------------------------------------------------------------------------------------------

def test_constant_source_window_model():
    ref = LS.oracle("const_window")[0]
    first, end = LS.window_frames(LS.CONST_START, LS.CONST_STOP, LS.L1)
    # Start(0.5) is frame 24,000 = block 187 + 64 on paper; the accumulated time of block 187 lies an ulp below 187 * 128 / sr, so
    # ceil((0.5 - t0) * sr) is 65: the reference starts one frame late, and so must every renderer
    assert first == 24001 and end == 2100 * B + 40 and ref[first] != 0 and ref[end - 1] != 0
    assert not ref[:first].any() and not ref[end:].any()
    frames = np.arange(0, FRAMES, LS.STRIDE)
    assert len(set(frames % B)) == B
    want = LS.timeline_at(LS.const_timeline(), frames, LS.L1)
    want[(frames < first) | (frames >= end)] = 0.0
    assert np.array_equal(ref[frames], want)
    assert len(np.unique(want)) > 1000


# ---- the two oracles, as the GPU file assumes them ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["osc_curve", "osc_curve_as_offset", "delay_ramp"])
def test_no_libm_in_scenes_2_and_7(name):
    a, d = LS.oracle(name), LS.dtrig(name)
    assert np.isfinite(a).all() and G.rms(a) > 1e-3
    assert np.array_equal(a, d)


@pytest.mark.parametrize("name", ["pan_long_stereo", "pan_long_mono", "pan_carried_held", "pan_carried_returned", "bq_long", "krate_mod"])
def test_double_trig_references_of_scenes_9_and_10(name):
    d = LS.dtrig(name)
    assert np.isfinite(d).all() and G.rms(d) > 1e-3 and np.abs(d).max() < 10.0
    a = LS.oracle(name)
    print(f"{name}: plain vs double-trig oracle rms {G.rms(a - d):.3e}, max {float(np.abs(a - d).max()):.3e}")
    assert np.isfinite(a).all() and G.rms(a) > 1e-3


def test_k_rate_modulation_is_heard():
    flat, _ = LS.render(OracleContext, LS.krate_mod(0.0))
    mod = LS.oracle("krate_mod")
    per_block = np.abs(mod[0] - flat[0]).reshape(LS.L1, B).max(axis=1)
    assert G.rms(mod - flat) > 1e-3 and (per_block[2048:] > 1e-4).mean() > 0.9


def test_panner_changes_where_the_scene_says():
    tl = LS.pan_long_timeline()
    blocks = sorted(set(LS.PAN_LONG_CHANGES + [2176]))
    frames = np.array(sorted({b * B + k for b in blocks for k in (0, B - 1)} | {(b + 1) * B for b in blocks}))
    p = LS.timeline_at(tl, frames, LS.L1)
    at = dict(zip(frames.tolist(), p.tolist()))
    for b in LS.PAN_LONG_CHANGES:    # a change inside the block: its first and last frame differ
        assert at[b * B] != at[b * B + B - 1], b
    assert at[2176 * B] == np.float32(0.6) and at[2175 * B + B - 1] == np.float32(-0.25)
    ramp = LS.timeline_at(tl, np.arange(0, 300 * B, LS.STRIDE), LS.L1)
    assert (ramp < 0).sum() > 100 and (ramp > 0).sum() > 100


def blocks_equal(a, b):
    return (a.reshape(a.shape[0], -1, B) == b.reshape(b.shape[0], -1, B)).all(axis=(0, 2))


def test_panner_scenes_in_which_only_the_carried_state_tells():
    """On the oracle: which blocks run on gains that are no function of the pan.  held: every block up to the change in block 2110
    still carries block 0's stereo-law gains.  returned: blocks 1 .. 9 do; from block 21 on the pan is 0.5 again, with the mono
    law's gains."""
    held, held_mono = LS.dtrig("pan_carried_held"), LS.dtrig("pan_carried_held_mono")
    eq = blocks_equal(held, held_mono)
    assert not eq[1:LS.PAN_HELD_UNTIL].any() and eq[LS.PAN_HELD_UNTIL + 1:].all()
    back, back_mono = LS.dtrig("pan_carried_returned"), LS.dtrig("pan_carried_returned_mono")
    eq = blocks_equal(back, back_mono)
    assert not eq[1:10].any() and eq[21:].all()
    assert not blocks_equal(back, held)[21:LS.PAN_HELD_UNTIL].any()      # the same pan, other gains
    for name in ("pan_carried_held", "pan_carried_returned"):             # steps only: one trig argument per change
        assert np.array_equal(LS.oracle(name), LS.dtrig(name))


def test_delay_onset_control():
    """The scene can detect an early flag, on the oracle alone: with the leading zeros replaced by 1e-30 -- what a prediction from the
    input's flags takes them for -- the biquad is never frozen and the output moves."""
    a, c = LS.oracle("delay_onset")[0], LS.oracle("delay_onset_control")[0]
    onset = int(np.flatnonzero(LS.oracle("delay_onset")[0][1170 * B:])[0]) + 1170 * B
    print(f"delay onset: first non-zero output behind the burst at frame {onset} = block {onset // B}")
    assert onset // B > 1170 + 4                                         # frozen for blocks in between
    assert not a[(LS.ONSET_BURST_BLOCK + 4) * B:(onset // B) * B].any()  # ... and silent there
    moved = G.rms(a[LS.ONSET_WINDOW] - c[LS.ONSET_WINDOW])
    assert moved >= 1e-3, moved
