"""The "libm class" (DESIGN.md section 8), pinned on the CPU: the oracle against the same oracle built with the device's evaluation
of cos / sin / pow ((float)cos((double)x) where the reference has cosf; DtrigOracleContext).  For every scene family of
tests/test_gpu_param_edges.py: the class is small (one `LIBMCLASS` line per scene: RMS, max-abs, share of differing samples; the
table in DESIGN.md is made from these lines), and scenes marked `exact` -- steps, whose few trig arguments agree between the two
evaluations -- are bit-equal between the two oracles, which is what lets the GPU tests compare the device with the PLAIN oracle for
them.  Last: NaN through the Q clamp of BiQuadFilterNode (Math.Max keeps it), the expectation written out from the C#."""
import numpy as np
import pytest

from tests import _graphs as G
from tests import _param_scenes as P
from tests._oracle import DtrigOracleContext, OracleContext

SCENES = P.biquad_scenes() + P.panner_scenes() + [P.bq_nan_f()]
FENCE = 1e-6   # a sanity fence above the largest class measured for a non-resonant scene (3.3e-7: 80 biquads); not a tuned bound


@pytest.mark.parametrize("scene", SCENES, ids=repr)
def test_libm_class_of_scene(scene):
    plain = P.render(OracleContext, scene)
    dtrig = P.render(DtrigOracleContext, scene)
    rms, mx, share = P.libm_class(plain, dtrig)
    print(f"LIBMCLASS {scene.name}: signal rms {G.rms(plain):.3e}  plain vs double-trig rms {rms:.2e}  max {mx:.2e}  "
          f"differing {100 * share:.2f} %{'  (amplified)' if scene.amplified else ''}")
    assert np.isfinite(plain).all() and np.isfinite(dtrig).all()
    assert G.rms(plain) > 1e-3 and np.abs(plain).max() < 10.0
    if scene.exact:
        assert np.array_equal(plain, dtrig)
    elif scene.amplified:
        assert FENCE < rms <= 1e-5   # (above the fence, or it would not belong on this list; inside the contract bound)
    else:
        assert rms <= FENCE


@pytest.mark.parametrize("scene", [s for s in SCENES if s.exact or s.edits], ids=repr)
def test_oracle_renders_the_same_in_pieces(scene):
    """The uneven pieces of the GPU tests are no different render on the oracle (it works block by block)."""
    assert np.array_equal(P.render(OracleContext, scene), P.render(OracleContext, scene, "chunk5"))


# ---- NaN through Math.Max(0.001f, q) (BiQuadFilterNode.cs:124) ----------------------------------------------------------------

@pytest.mark.parametrize("mk", [OracleContext, DtrigOracleContext], ids=["plain", "dtrig"])
def test_nan_q_with_the_frequency_held_changes_nothing(mk):
    """q = NaN: `|q - usedQ| > 0.0001` is false and the frequency (1800 Hz, updated at the block's first sample) has not moved: no
    update at the NaN frames, the coefficients of the frame before stay.  The same render with the modulator's NaN frames replaced
    by the value of the frame before them (q == usedQ: no update either) must be identical.  An implementation that turns the NaN
    into 0.001 updates there and differs."""
    out = P.render(mk, P.bq_nan_q(False))
    assert np.isfinite(out).all() and G.rms(out) > 1e-3
    assert np.array_equal(out, P.render(mk, P.bq_nan_q(False, held=True)))


@pytest.mark.parametrize("mk", [OracleContext, DtrigOracleContext], ids=["plain", "dtrig"])
def test_nan_q_with_the_frequency_moving_makes_the_coefficients_nan(mk):
    """The frequency ramps by 0.01 Hz per sample: every sample updates.  At the first NaN frame (300) the update computes
    alpha = sin / (2 * NaN): every coefficient is NaN, w = x - a1 * W1 - a2 * W2 is NaN and stays in the state: every sample from
    frame 300 on is NaN, in both channels (channel 1 enters its loop with the finite coefficients of frame 383 and meets the same NaN
    at its own frame 300), up to the block in which the source ends."""
    out = P.render(mk, P.bq_nan_q(True))
    first = P.NAN_Q_FRAMES[0]
    assert np.isfinite(out[:, :first]).all() and G.rms(out[:, :first]) > 1e-3
    assert np.isnan(out[:, first:23 * P.B]).all()


@pytest.mark.parametrize("mk", [OracleContext, DtrigOracleContext], ids=["plain", "dtrig"])
def test_nan_frequency_is_kept_by_the_clamp_and_updates_nothing(mk):
    """Math.Clamp keeps a NaN frequency; `|NaN - usedFreq| > 0.001` is false and Q is constant: the NaN frames pass with the
    coefficients of the frame before.  The same render with each NaN replaced by the value of the frame before it (f == usedFreq:
    no update either) is identical.  A clamp that turned the NaN into a bound would update there and differ."""
    out = P.render(mk, P.bq_nan_f())
    assert np.isfinite(out).all() and G.rms(out) > 1e-3
    assert np.array_equal(out, P.render(mk, P.bq_nan_f(held=True)))


@pytest.mark.parametrize("mk", [OracleContext, DtrigOracleContext], ids=["plain", "dtrig"])
def test_constant_nan_q(mk):
    """Q written to NaN by the Value setter after four blocks.  At 1000 Hz no condition of the update holds any more: the render
    equals the one without the write.  At 1800 Hz the next block's first sample updates (the frequency is off the baseline) with
    alpha = sin / (2 * NaN): NaN from that block on, also behind a convolver."""
    at = P.bq_constant_nan_q(1000.0)
    out = P.render(mk, at)
    assert np.isfinite(out).all() and G.rms(out[:, P.NAN_Q_SET_AT:]) > 1e-3
    assert np.array_equal(out, P.render(mk, P.bq_constant_nan_q(1000.0, with_nan=False)))
    for scene in (P.bq_constant_nan_q(1800.0), P.bq_constant_nan_q(1800.0, behind_convolver=True)):
        out = P.render(mk, scene)
        assert np.isfinite(out[:, :P.NAN_Q_SET_AT]).all() and G.rms(out[:, :P.NAN_Q_SET_AT]) > 1e-3
        assert np.isnan(out[:, P.NAN_Q_SET_AT:11 * P.B]).all()


# ---- the delay curves stay clear of the integers; the parameter restatement agrees with the oracle ---------------------------

@pytest.mark.parametrize("kind,max_delay,nch,neg", P.DELAY_CASES)
def test_delay_curves_stay_clear_of_integer_crossings(kind, max_delay, nch, neg):
    curve = P.delay_timeline(kind, max_delay).curve(24 * P.B)
    dist = P.integer_distance(P.delay_samples(curve))
    assert ((dist >= 1e-3) | (dist == 0)).all()
    assert np.array_equal(P.render(OracleContext, P.delay_scene(kind, max_delay, nch, neg)),
                          P.render(DtrigOracleContext, P.delay_scene(kind, max_delay, nch, neg)))


def ulps(a, ref):
    return np.abs(a.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("name,edit", [(n, None) for n in P.PARAM_TIMELINES] + [(None, e) for e in P.PARAM_EDITS])
def test_parameter_restatement_agrees_with_the_oracle(name, edit):
    out = P.render(OracleContext, P.param_scene(name, edit))
    want = P.param_expected(name, out.shape[1], edit)
    if P.param_has_exp(name, edit):
        assert ulps(out[0], want).max() <= 2 and ulps(out[1], want).max() <= 2
    else:
        assert np.array_equal(out[0], want) and np.array_equal(out[1], want)
    assert len(np.unique(want)) > 100 or name == "late_base_step" or (edit and P.PARAM_EDITS[edit][0] == "late_base_step")
