"""Option "libm_exact" (libm class): with it biquad_dynamic_kernel and stereo_panner_dynamic_kernel evaluate
cosf / sinf / powf as glibc does (graphaudio_amd/csrc/ga_libmf.hpp) instead of the double-precision functions rounded once, so the
reference of the moving-parameter scenes is the PLAIN oracle -- the contract -- and the condition is np.array_equal.  Without the
option the device meets that only on scenes marked `exact`; tests/test_gpu_param_edges.py holds the default path against the
double-trig oracle and stays as it is.

Every scene that is not `exact` first shows on the CPU that the plain and the double-trig oracle differ on it: the device cannot pass
by evaluating what it evaluates by default.  Oracle renders are made once per (scene, form) and shared."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from graphaudio_amd import ArgumentException, ArgumentOutOfRangeException, FilterType, OfflineAudioContext
from tests import _graphs as G
from tests import _libm_scenes as L
from tests import _param_scenes as P
from tests._oracle import DtrigOracleContext, OracleContext

B = P.B
FORMS = P.BOTH_FORMS

_oracle = {}


def oracle(mk, scene, form):
    key = (mk.__name__, scene.name, form)
    if key not in _oracle:
        _oracle[key] = P.render(mk, scene, form)
        _oracle[key].setflags(write=False)
    return _oracle[key]


def hold_against_the_plain_oracle(scene, form):
    ref = oracle(OracleContext, scene, form)
    assert np.isfinite(ref).all() and G.rms(ref) > 1e-3 and np.abs(ref).max() < 10.0
    if not scene.exact:
        dtrig = oracle(DtrigOracleContext, scene, form)
        assert not np.array_equal(ref, dtrig), (scene.name, form, "the two oracles agree: the scene does not tell cosf from the rounded-once double")
    got = P.render(L.exact_context(form), scene, form)
    bad = np.flatnonzero((ref != got).any(axis=0))
    assert np.array_equal(ref, got), (scene.name, form, "first differing frames", bad[:6], "of", len(bad), "max", float(np.abs(ref - got).max()))
    return ref


# ---- the option's surface ------------------------------------------------------------------------------------------------------

def test_values_other_than_0_and_1_are_out_of_range():
    h = OfflineAudioContext(P.SR)
    h.SetOption("libm_exact", 0)
    h.SetOption("libm_exact", 1)
    for bad in (2, -1):
        with pytest.raises(ArgumentOutOfRangeException):
            h.SetOption("libm_exact", bad)
    with pytest.raises(ArgumentException) as e:   # (an unknown key is an invalid argument, not a range error)
        h.SetOption("libm_exact_", 1)
    assert not isinstance(e.value, ArgumentOutOfRangeException)
    h.Dispose()


# ---- scenes on which the two oracles differ --------------------------------------------------------------------------------------

def k_and_a_rate_scene():
    """The scene of test_gpu_param_edges.py::test_k_rate_and_a_rate_sampling_of_one_timeline: one ramp on the gain (k-rate) and the
    frequency (a-rate) of a high-shelf."""
    def build(ctx):
        s = P.noise(ctx, 2, 30, scale=0.05)
        bq = P.biquad(ctx, FilterType.Highshelf, s, f=P.ftl().set(2000.0, 0.0).lin(2012.0, 25.5 * B / P.SR), qv=1.2,
                      g=P.gtl().set(-12.0, 0.0).lin(12.0, 25.5 * B / P.SR))
        bq.Connect(ctx.Destination)
        return (s, bq)
    return P.Scene("k_and_a_rate", build, 30)


BIQUAD_SCENES = ([P.bq_slow_ramp(*r) for r in P.SLOW_RAMPS]
                 + [P.bq_slow_ramp("slow_0004", 500.0, 0.0004, FilterType.Peaking, nch=3, qv=2.0),
                    P.bq_slow_ramp("through_1000", 999.9, 0.00003, FilterType.Allpass, nch=3), P.bq_exp_ramp(),
                    P.bq_q_ramp(FilterType.Lowpass, True), P.bq_type_written(), P.bq_input_falls_silent(), P.bq_modulated(), P.bq_crowd(),
                    k_and_a_rate_scene()])
PANNER_SCENES = [P.pan_ramp("stereo"), P.pan_ramp("mono"), P.pan_crowd()]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scene", BIQUAD_SCENES, ids=repr)
def test_automated_biquad_equals_the_plain_oracle(scene, form):
    assert not scene.exact
    hold_against_the_plain_oracle(scene, form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scene", PANNER_SCENES, ids=repr)
def test_automated_panner_equals_the_plain_oracle(scene, form):
    """pan_ramp: the per-sample pass computes the gains; pan_crowd and the chunked form also carry them from block to block
    through the lane-0 pass and the node's state."""
    assert not scene.exact
    hold_against_the_plain_oracle(scene, form)


# ---- the plumbing: scenes on which the two oracles agree, with the option on -------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scene", [P.bq_steps(FilterType.Lowpass), P.bq_steps(FilterType.Highshelf), P.bq_gain_ramp(FilterType.Peaking, False),
                                   P.pan_steps("stereo"), P.pan_group_state()], ids=repr)
def test_exact_scenes_stay_exact_with_the_option_on(scene, form):
    assert scene.exact
    hold_against_the_plain_oracle(scene, form)


# ---- powf ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("ftype", L.POW_TYPES, ids=lambda t: t.name)
def test_gain_steps_through_values_where_powf_is_not_the_rounded_double(ftype, form):
    g = L.pow_gain_timeline().curve(L.POW_BLOCKS * B, arate=False)
    assert g[0] == 0.0 and all(np.all(g[(k + 1) * B:(k + 2) * B] == L.POW_GAINS[k]) for k in range(24)) and g[-1] == L.POW_GAINS[-1]
    assert np.all((L.POW_GAINS >= -60.0) & (L.POW_GAINS <= 60.0))
    hold_against_the_plain_oracle(L.pow_scene(ftype), form)   # (asserts that the two oracles differ)


# ---- the two fuzz sessions of the class (tests/test_gpu_fuzz.py::test_documented_open_seed keeps them as xfails, option off) ---------

@pytest.mark.parametrize("seed", [30228, 60235])
def test_fuzz_session_of_the_libm_class_meets_its_bound(seed):
    """The options of test_gpu_fuzz._session_pair plus libm_exact = 1, at the bounds of test_documented_open_seed.  Measured on MI355X:
    30228 2.6e-8 rms against the plain oracle (1.96e-2 with the option off, 2.8e-8 against the double-trig oracle), 60235 bit-identical."""
    from tests._fuzz import run_random_session
    o = OracleContext(48000)
    ref, ref_log = run_random_session(o, seed)
    h = OfflineAudioContext(48000)
    h.SetOption("max_chunk_blocks", 11)
    h.SetOption("coarse_min_blocks", 1 << 30)
    h.SetOption("coarse_tail", 1)
    h.SetOption("coarse_premix", 1)
    h.SetOption("coarse_tail_private", 0)
    h.SetOption("libm_exact", 1)
    got, got_log = run_random_session(h, seed)
    assert ref_log == got_log
    err = G.rms(ref - got)
    scale = max(G.rms(ref), 1e-3)
    per_block = [G.rms(ref[:, b * B:(b + 1) * B] - got[:, b * B:(b + 1) * B]) for b in range(ref.shape[1] // B)]
    worst = int(np.argmax(per_block))
    print(f"session {seed}: rms error against the plain oracle {err:.3e} (signal {scale:.3e}), {int((ref != got).sum())} of {ref.size} values differ, "
          f"worst block {worst}: {per_block[worst]:.3e}")
    assert err <= 1e-5 * max(1.0, scale if seed >= 50000 else 1.0) and err <= 2e-5 * scale, (seed, err, scale)
