"""The kernels that evaluate MOVING parameters, one node kind per test, bit for bit: biquad_dynamic_kernel,
stereo_panner_dynamic_kernel, delay_kernel with a moving delay time, param_curve_kernel and param_mod_kernel.

The device evaluates cos / sin / pow as (float)cos((double)x) where the reference has cosf ("libm class"), so the
reference here is the double-trig oracle (DtrigOracleContext: that evaluation, everything else the reference's) and the condition is
np.array_equal.  Scenes marked `exact` (tests/_param_scenes.py; proven bit-equal between the two oracles by
tests/test_oracle_libm_class.py) are held against the plain oracle as well.  Every case renders as one piece and in uneven pieces of
5-block chunks, and first proves -- on the oracle's output or on the parameter curve recomputed in numpy -- that the edge it
targets occurs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from graphaudio_amd import FilterType, OfflineAudioContext
from tests import _graphs as G
from tests import _param_scenes as P
from tests._oracle import DtrigOracleContext, OracleContext

B = P.B
FORMS = P.BOTH_FORMS


def hold_bit_for_bit(scene, form, nan=False):
    """device == double-trig oracle; for an exact scene also == plain oracle.  Returns the double-trig oracle's render."""
    ref = P.render(DtrigOracleContext, scene, form)
    if not nan:
        assert np.isfinite(ref).all() and G.rms(ref) > 1e-3 and np.abs(ref).max() < 10.0
    got = P.render(OfflineAudioContext, scene, form)
    bad = np.flatnonzero((ref != got).any(axis=0) & ~(np.isnan(ref) & np.isnan(got)).all(axis=0))
    assert np.array_equal(ref, got, equal_nan=nan), (scene.name, form, "first differing frames", bad[:6], "of", len(bad),
                                                     "max", float(np.nanmax(np.abs(ref - got))))
    if scene.exact:
        assert np.array_equal(P.render(OracleContext, scene, form), got, equal_nan=nan)
    return ref


def blocks_rms(x):
    return [G.rms(x[:, b * B:(b + 1) * B]) for b in range(x.shape[1] // B)]


# ---- BiQuadFilterNode --------------------------------------------------------------------------------------------------------

def test_edge_frequency_steps_and_the_per_block_baseline():
    """On the curve: which blocks update how often.  Block 4 steps to exactly 1000 Hz at Q 1: NO update (usedFreq starts every
    block at 1000), the 3000 Hz coefficients stay through 999.9995 and 1000.0009; 1000.002 is outside the hysteresis."""
    f = P.step_f_timeline().curve(P.STEP_BLOCKS * B)
    n = P.biquad_updates(f, np.ones_like(f))
    assert f[4 * B] == 1000.0 and f[6 * B + 37] == np.float32(999.9995) and f[8 * B] == np.float32(1000.0009)
    assert n[0] == 1 and n[4:10] == [0] * 6 and n[10] == 1 and n[11] == 1
    assert f[14 * B + 3] == 24000.0 and f[16 * B + 100] == 24000.0 and n[14] == 3 and n[16] == 3   # Nyquist, and 30000 clamped to it
    assert f[21 * B] == 1.0 and f[22 * B + 5] == 1.0 and f[23 * B + 77] == 1.0 and n[22] == n[23] == 1   # 0 and -5: the lower clamp, no new value
    # block 28: 440 at its start (one update: every block starts from the 1000 baseline), 1000 from frame 1 (a second: usedFreq is
    # 440 by then); block 29 starts at 1000: none until 2500 at frame 127
    assert n[28] == 2 and n[29] == 1 and f[29 * B] == 1000.0


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("ftype", P.CROWD_TYPES, ids=lambda t: t.name)
def test_biquad_frequency_steps(ftype, form):
    ref = hold_bit_for_bit(P.bq_steps(ftype), form)
    if ftype == FilterType.Lowpass:   # the edge on the output: blocks 4..9 are filtered with the 3000 Hz coefficients, not 1000 Hz ones
        r = blocks_rms(ref)
        assert min(r[4:10]) > 0.75 * r[2] and r[11] < 0.9 * r[2]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name,f0,slope", P.SLOW_RAMPS)
def test_biquad_slow_ramp(name, f0, slope, form):
    """Under 0.001 Hz per sample the update is a sequential decision every few samples."""
    f = P.ramp_f_timeline(f0, slope, P.RAMP_BLOCKS).curve(P.RAMP_BLOCKS * B)
    n = P.biquad_updates(f, np.ones_like(f), nch=2)
    assert 2 <= min(n) and max(n) <= 127 * 2, (min(n), max(n))
    one = P.biquad_updates(f, np.ones_like(f), nch=1)
    assert 2 <= min(one) and max(one) <= 127, (min(one), max(one))
    if name == "through_1000":   # blocks that start inside the hysteresis of the 1000 Hz baseline: no update at their first sample
        starts = [b for b in range(P.RAMP_BLOCKS) if abs(np.float32(f[b * B] - np.float32(1000.0))) <= np.float32(0.001)]
        assert len(starts) >= 1
    hold_bit_for_bit(P.bq_slow_ramp(name, f0, slope), form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scene", [P.bq_slow_ramp("slow_0004", 500.0, 0.0004, FilterType.Peaking, nch=3, qv=2.0),
                                   P.bq_slow_ramp("through_1000", 999.9, 0.00003, FilterType.Allpass, nch=3), P.bq_exp_ramp()], ids=repr)
def test_biquad_ramps_three_channels_and_exponential(scene, form):
    ref = hold_bit_for_bit(scene, form)
    assert all(G.rms(ref[c]) > 1e-3 for c in range(min(scene.ch, 3)))


def test_edge_q_steps():
    q = P.q_step_timeline().curve(20 * B)
    f = P.ftl().set(700.0, 0.0).set(1000.0, P.at_frame(B)).curve(20 * B)
    n = P.biquad_updates(f, q)
    # 1.00005 / 0.99995 / 1.00009: inside the 0.0001 hysteresis around 1 -- no update; 1.0002 / 0.99985: outside; 0.0005 and -3: both
    # the parameter's minimum 0.001, one value; 700 is inside the range
    assert q[7 * B] == np.float32(0.001) and q[9 * B + 64] == np.float32(0.001)
    assert n[1:5] == [0, 0, 0, 0] and n[5] == 1 and n[6] == 1 and n[7] == 1 and n[9] == 1 and n[13] == 2 and n[14] == 0
    assert n[15] == 1 and n[17] == 2 and n[18] == 0 and n[19] == 0


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("ftype", [FilterType.Lowpass, FilterType.Notch, FilterType.Highshelf], ids=lambda t: t.name)
def test_biquad_q_steps(ftype, form):
    hold_bit_for_bit(P.bq_q_steps(ftype), form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scene", [P.bq_q_ramp(FilterType.Bandpass, False), P.bq_q_ramp(FilterType.Lowpass, True)], ids=repr)
def test_biquad_q_ramp(scene, form):
    """Q ramps by 2e-3 per sample: an update at every sample.  The scene with the frequency moving as well is "amplified": the
    device is held bit for bit against the double-trig oracle, and that is the whole condition (against the plain oracle the
    leg device-vs-plain would be the CPU-only quantity plain-vs-double-trig, an identity)."""
    q = P.qtl().set(0.5, 0.0).lin(8.0, 30 * B / P.SR).curve(40 * B)
    f = P.ramp_f_timeline(300.0, 0.02, 40).curve(40 * B) if scene.amplified else np.full(40 * B, 700.0, np.float32)
    n = P.biquad_updates(f, q)
    # an update at every sample while Q ramps (blocks 0..29); after it one per block (700 Hz is off the baseline) or, with the
    # frequency still moving by 0.02 Hz per sample, still every sample
    assert n[:30] == [B] * 30 and n[31:] == [B if scene.amplified else 1] * 9
    hold_bit_for_bit(scene, form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("beyond", [False, True])
@pytest.mark.parametrize("ftype", [FilterType.Peaking, FilterType.Lowshelf, FilterType.Highshelf], ids=lambda t: t.name)
def test_biquad_gain_ramp(ftype, beyond, form):
    g = P.gtl().set(-30.0, 0.0).lin(30.0, 36 * B / P.SR).curve(40 * B, arate=False)
    assert len(np.unique(g)) == 37 and all(len(np.unique(g[b * B:(b + 1) * B])) == 1 for b in range(40))   # k-rate: one value per block
    if beyond:   # -30 .. 30 with -50 / +50 added: below -60 in the first blocks, above 60 in the last ones
        assert g[0] - 50.0 < -60.0 and g[39 * B] + 50.0 > 60.0
    ref = hold_bit_for_bit(P.bq_gain_ramp(ftype, beyond), form)
    r = blocks_rms(ref)
    assert r[38] > 2 * r[1]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nch", [2, 3])
def test_biquad_used_frequency_carries_from_channel_to_channel(nch, form):
    tl = P.ftl()
    for b in range(20):
        tl.set(1000.0, P.at_frame(b * B)).set(2000.0, P.at_frame(b * B + 64))
    f = tl.curve(20 * B)
    # one update per block for one channel (to 2000 at frame 64; the block's start sits on the baseline), 2 more per further channel
    assert P.biquad_updates(f, np.ones_like(f), 1)[1:] == [1] * 19 and P.biquad_updates(f, np.ones_like(f), nch)[1:] == [2 * nch - 1] * 19
    ref = hold_bit_for_bit(P.bq_channel_carry(nch), form)
    # the same input on every channel, but channel 0 differs from channel 1 (and channel 2 from both: its state took another path)
    assert G.rms(ref[0] - ref[1]) > 1e-3
    if nch == 3:
        assert G.rms(ref[2]) > 1e-3 and G.rms(ref[0] - ref[2]) > 1e-3


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scene", [P.bq_mono_becomes_stereo(), P.bq_type_written(), P.bq_automation_ends_and_returns(),
                                   P.bq_input_falls_silent(), P.bq_modulated()], ids=repr)
def test_biquad_graph_changes_under_automation(scene, form):
    ref = hold_bit_for_bit(scene, form)
    r = blocks_rms(ref)
    if scene.name == "bq_mono_becomes_stereo":     # both channels the same up to the block in which the stereo source starts
        assert np.array_equal(ref[0, :16 * B], ref[1, :16 * B]) and G.rms(ref[0, 18 * B:] - ref[1, 18 * B:]) > 1e-3
    elif scene.name == "bq_input_falls_silent":    # exact silence between the sources, sound before and after
        assert min(r[:12]) > 1e-3 and not ref[:, 14 * B:25 * B].any() and min(r[27:44]) > 1e-3
    elif scene.name == "bq_type_written":          # the low-shelf written at block 30 on the 1000 Hz plateau sounds different from the notch
        plain_notch = P.Scene("no_last_edit", scene.build, 40, edits={k: v for k, v in list(scene.edits.items())[:3]})
        other = P.render(DtrigOracleContext, plain_notch, form)
        assert np.array_equal(ref[:, :30 * B], other[:, :30 * B]) and G.rms(ref[:, 30 * B:] - other[:, 30 * B:]) > 1e-3
    elif scene.name == "bq_modulated":
        # on the curves: the modulators end inside blocks 26 (3,333 frames) and 16 (2,100 frames); the rest of that block the
        # modulation is 0 (the block is not silent), from the next block on the parameters are their intrinsic values.  Up to there
        # every sample updates, from block 27 on one update per block (1500 Hz is off the baseline)
        mf, mq = np.zeros(45 * B, np.float32), np.zeros(45 * B, np.float32)
        mf[:3333] = P.modulator_signal(3333, 41) * np.float32(900.0)
        mq[:2100] = P.modulator_signal(2100, 43, 333.0) * np.float32(1.5)
        f = np.clip(np.float32(1500.0) + mf, np.float32(1.0), np.float32(P.NYQ))
        q = np.clip(np.float32(2.0) + mq, np.float32(0.001), np.float32(1000.0))
        n = P.biquad_updates(f, q)
        assert 3333 // B == 26 and 2100 // B == 16 and min(n[:26]) == B and 1 < n[26] < B and n[27:] == [1] * 18
        assert (q[:2100] != 2.0).mean() > 0.99 and np.all(q[2100:] == 2.0) and np.all(f[3333:] == 1500.0)
        assert min(r[:44]) > 1e-3
    elif scene.name == "bq_automation_ends_and_returns":
        # on the oracle: the Value write (seen from block 16 on) changes the render from there, and not before; the timeline
        # scheduled at block 36 changes it from block 40 (its first event) on, and not before
        none = P.render(DtrigOracleContext, P.bq_automation_ends_and_returns(upto=0), form)
        first = P.render(DtrigOracleContext, P.bq_automation_ends_and_returns(upto=1), form)
        assert np.array_equal(ref[:, :16 * B], none[:, :16 * B]) and G.rms(ref[:, 16 * B:20 * B] - none[:, 16 * B:20 * B]) > 1e-3
        assert np.array_equal(ref[:, :40 * B], first[:, :40 * B]) and G.rms(ref[:, 40 * B:] - first[:, 40 * B:]) > 1e-3
        # and on the curve: between the two the frequency is the constant 620 Hz (one update per block), moving before and after
        f = np.concatenate([P.ramp_f_timeline(300.0, 0.05, 20).curve(16 * B), np.full(24 * B, 620.0, np.float32),
                            P.ftl(620.0).set(620.0, 40 * B / P.SR).lin(200.0, 55 * B / P.SR).curve(60 * B)[40 * B:]])
        n = P.biquad_updates(f, np.full(60 * B, 3.0, np.float32))
        assert min(n[:16]) == B and n[16:40] == [1] * 24 and min(n[40:55]) == B


@pytest.mark.parametrize("form", FORMS)
def test_80_automated_biquads_in_one_level(form):
    for v in range(80):   # per voice, on its curves: the coefficient updates
        ftl_, qtl_ = P.bq_crowd_timelines(v)
        f = ftl_.curve(24 * B) if ftl_ else np.full(24 * B, 900.0 + 13 * v, np.float32)
        q = qtl_.curve(24 * B) if qtl_ else np.ones(24 * B, np.float32)
        n = P.biquad_updates(f, q)
        if v % 3 == 0:   # steps: one update per block, none in the blocks at exactly 1000 Hz and Q 1, one per block again after them
            assert n[0] == 1 and 0 in n[3:14] and n[-1] == 1, (v, n)
        else:            # ramps of the frequency or of Q: several updates per block while they run
            assert sum(n) >= 24 * 2, (v, sum(n))
    ref = hold_bit_for_bit(P.bq_crowd(), form)
    assert all(G.rms(ref[c]) > 1e-3 for c in range(32))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scene", P.nan_scenes(), ids=repr)
def test_biquad_nan_parameters(scene, form):
    """Math.Max keeps a NaN Q, Math.Clamp a NaN frequency (tests/test_oracle_libm_class.py writes the expectation out): NaN
    positions equal, everything else bit for bit."""
    if scene.name.endswith("convolver"):
        # a convolver's output is within 2e-6 relative of the oracle's, not bit-equal: NaN positions equal, the finite blocks close
        ref = P.render(DtrigOracleContext, scene, form)
        got = P.render(OfflineAudioContext, scene, form)
        assert np.array_equal(np.isnan(ref), np.isnan(got))
        fin = ~np.isnan(ref)
        assert G.rms(ref[fin]) > 1e-3 and G.rms(ref[fin] - got[fin]) <= 2e-6 * G.rms(ref[fin])
    else:
        ref = hold_bit_for_bit(scene, form, nan=True)
    if scene.name == "bq_nan_q_moving_f":
        assert np.isfinite(ref[:, :300]).all() and np.isnan(ref[:, 300:23 * B]).all()
    elif scene.name.startswith("bq_constant_nan_q_1800"):   # the Value setter wrote NaN at block 4: NaN from there on
        assert np.isfinite(ref[:, :P.NAN_Q_SET_AT]).all() and np.isnan(ref[:, P.NAN_Q_SET_AT:11 * B]).all()
    else:
        assert np.isfinite(ref).all() and G.rms(ref) > 1e-3
    plain = P.render(OracleContext, scene, form)
    assert np.array_equal(np.isnan(plain), np.isnan(ref))


# ---- StereoPannerNode --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("law", ["stereo", "mono", "quirk"])
def test_panner_steps_through_zero_and_beyond_the_range(law, form):
    p = P.pan_step_timeline().curve(22 * B)
    assert p[10 * B] == 1.0 and p[13 * B] == -1.0 and p[8 * B + 1] == 1.0   # 1.5 and -2 are clamped; 1.0 -> 1.5 is no change
    assert p[4 * B + 33] == 0.0 and p[4 * B + 32] == -0.5
    ref = hold_bit_for_bit(P.pan_steps(law), form)
    assert np.array_equal(ref[1, :2 * B], np.zeros(2 * B, np.float32)) or law == "stereo"   # pan -1: nothing on the right (mono laws)
    if law == "quirk":   # block 0 runs the stereo law on the up-mixed mono buffer, later blocks the mono law with the gains of block 0
        mono = P.render(DtrigOracleContext, P.pan_steps("mono"), form)
        assert not np.array_equal(ref[:, :B], mono[:, :B]) or not np.array_equal(ref[:, B:2 * B], mono[:, B:2 * B])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("law", ["stereo", "mono"])
def test_panner_ramp_through_zero_then_back_to_the_held_value(law, form):
    p = P.ptl().set(-1.0, 0.0).lin(1.0, 0.15).set(1.0, 60 * B / P.SR).lin(0.4, 64 * B / P.SR).set(0.4, 66 * B / P.SR).curve(70 * B)
    assert (p[:7000] < 0).sum() > 3000 and (p[:7000] > 0).sum() > 3000 and np.all(p[64 * B:] == np.float32(0.4))   # no recomputation from block 64 on
    hold_bit_for_bit(P.pan_ramp(law), form)


@pytest.mark.parametrize("form", list(P.FORMS))
@pytest.mark.parametrize("law", ["stereo", "mono"])
def test_panner_changes_at_the_edges_of_the_groups_of_64_blocks(law, form):
    """Where the pan changes, not what is carried: under these two laws the gains are a function of the pan, so a lost state
    heals at the next comparison -- the carried state is test_panner_state_carried_from_group_to_group's."""
    tl = P.ptl().set(0.5, 0.0)
    for k, b in enumerate(P.PAN_GROUP_CHANGES):
        tl.set([-0.5, 0.25, -0.75, 0.75, -0.25][k], P.at_frame(b * B + 17 * (k + 1)))
    p = tl.curve(140 * B)
    assert sorted(set(np.flatnonzero(p[1:] != p[:-1]) // B)) == P.PAN_GROUP_CHANGES
    hold_bit_for_bit(P.pan_group_edges(law), form)


@pytest.mark.parametrize("form", list(P.FORMS))
def test_panner_state_carried_from_group_to_group(form):
    """The hand-over of {last pan, gains} from one group of 64 blocks to the next (and, in chunks, through job.state), where it
    cannot heal: see P.pan_group_state."""
    p = P.pan_quirk_timeline().curve(140 * B)
    assert sorted(set(np.flatnonzero(p[1:] != p[:-1]) // B)) == [b for b, _ in P.PAN_QUIRK_CHANGES]
    assert np.all(p[:10 * B] == 0.5) and np.all(p[21 * B:66 * B] == 0.5) and np.all(p[101 * B:131 * B] == 0.5)
    ref = hold_bit_for_bit(P.pan_group_state(), form)
    mono = P.render(DtrigOracleContext, P.pan_group_state("mono"), form)
    # on the oracle: blocks 1..9 at pan 0.5 still carry block 0's stereo-law gains (they differ from the mono-law render, block by
    # block); blocks 21..65 and 101..130, at pan 0.5 again, carry the mono law's: the same pan, other gains
    assert all(not np.array_equal(ref[:, b * B:(b + 1) * B], mono[:, b * B:(b + 1) * B]) for b in range(1, 10))
    assert np.array_equal(ref[:, 21 * B:], mono[:, 21 * B:]) and G.rms(ref[:, 64 * B:66 * B]) > 1e-3 and G.rms(ref[:, 128 * B:131 * B]) > 1e-3


@pytest.mark.parametrize("form", FORMS)
def test_80_automated_panners(form):
    for v in range(80):   # per voice, on its curve: the pan moves -- two steps, or a ramp of hundreds of values (voice 40: 0 to 0)
        p = P.pan_crowd_timeline(v).curve(20 * B)
        changes = int((p[1:] != p[:-1]).sum())
        assert changes == 2 if v % 3 else (changes >= 100 or v == 40), (v, changes)
    hold_bit_for_bit(P.pan_crowd(), form)


# ---- DelayNode ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind,max_delay,nch,neg", P.DELAY_CASES)
def test_delay_with_a_moving_delay_time(kind, max_delay, nch, neg, form):
    curve = P.delay_timeline(kind, max_delay).curve(24 * B)
    prod = P.delay_samples(curve)
    dist = P.integer_distance(prod)
    assert ((dist >= 1e-3) | (dist == 0)).all()
    d = prod.astype(np.int64)
    top = int(np.float32(max_delay) * np.float32(P.SR))
    if kind == "steps":   # delay 0, the maximum (twice: once from beyond it), a jump across the write position (3 -> maximum)
        assert (d == 0).sum() > 3 * B and (d == top).sum() > 3 * B and d.max() == top and d[10 * B] - d[10 * B - 1] == top - 3
    else:                 # a read position that stands still (the delay grows by one sample every two frames) and one that runs at 1.5
        assert len(np.unique(d)) > 100
    scene = P.delay_scene(kind, max_delay, nch, neg)
    ref = hold_bit_for_bit(scene, form)
    if neg:               # the sum is negative in blocks 5..8: delay 0, silence
        assert not ref[:, 5 * B:9 * B].any()
    assert all(G.rms(ref[c]) > 1e-3 for c in range(min(nch, scene.ch)))


# ---- AudioParam timelines ----------------------------------------------------------------------------------------------------

def ulps(a, ref):
    return np.abs(a.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name,edit", [(n, None) for n in P.PARAM_TIMELINES] + [(None, e) for e in P.PARAM_EDITS])
def test_parameter_timeline(name, edit, form):
    """The curve itself is the output: a-rate through ConstantSourceNode.offset and GainNode.gain.  Steps and linear ramps bit for
    bit with both oracles and the float64 restatement; exp / pow curves (double-precision library calls on both sides) within
    2 float32 ulp of the restatement: one for the rounding to float of a double that may differ in its last bit, one for the
    restatement's own rounding.  `edit`: events cancelled, or ramps scheduled with an END BEFORE "now", between two render calls
    (P.PARAM_EDITS)."""
    scene = P.param_scene(name, edit)
    want = P.param_expected(name, scene.frames, edit)
    assert np.isfinite(want).all()
    if edit:   # the edge, on the restatement: the edit is seen from the next block on, as a jump or a changed course
        base, frame, ops = P.PARAM_EDITS[edit]
        cut = -(-frame // B) * B
        untouched = P.param_expected(base, scene.frames)
        assert np.array_equal(want[:cut], untouched[:cut]) and not np.array_equal(want[cut:], untouched[cut:])
        if edit.startswith("late"):
            assert all(op[2] < frame / P.SR for op in ops)                      # every end lies before "now"
            assert abs(float(want[cut]) - float(want[cut - 1])) > 0.1           # a jump at the block's start
            assert abs(float(want[cut]) - float(untouched[cut])) > 0.1
    else:
        assert len(np.unique(want)) > 100 or name == "late_base_step"
    ref = P.render(OracleContext, scene, form)
    got = P.render(OfflineAudioContext, scene, form)
    if P.param_has_exp(name, edit):
        for out in (ref, got):
            assert ulps(out[0], want).max() <= 2 and ulps(out[1], want).max() <= 2
    else:
        assert np.array_equal(ref[0], want) and np.array_equal(ref[1], want)
        assert np.array_equal(got, ref) and np.array_equal(got, P.render(DtrigOracleContext, scene, form))


@pytest.mark.parametrize("form", FORMS)
def test_k_rate_and_a_rate_sampling_of_one_timeline(form):
    """The same ramp on the gain (k-rate: the block's first value) and the frequency (a-rate) of a high-shelf."""
    def build(ctx):
        s = P.noise(ctx, 2, 30, scale=0.05)
        bq = P.biquad(ctx, FilterType.Highshelf, s, f=P.ftl().set(2000.0, 0.0).lin(2012.0, 25.5 * B / P.SR), qv=1.2,
                      g=P.gtl().set(-12.0, 0.0).lin(12.0, 25.5 * B / P.SR))
        bq.Connect(ctx.Destination)
        return (s, bq)
    g = P.gtl().set(-12.0, 0.0).lin(12.0, 25.5 * B / P.SR)
    assert len(np.unique(g.curve(30 * B, arate=False))) == 27 and len(np.unique(g.curve(30 * B))) > 3000
    hold_bit_for_bit(P.Scene("k_and_a_rate", build, 30), form)
