"""Known answers for tests/_compressor_model.py, the float64 model the DynamicsCompressorNode kernels are held to (DESIGN.md
section 2g).  No GPU needed."""
import numpy as np
import pytest

from tests import _compressor_model as M

FS = 48000


def _settled_level_db(level_db, **params):
    pars = M.block_params(FS, **params)
    x = np.full((1, 128 * 400), 10.0 ** (level_db / 20.0), dtype=np.float32)
    cm = M.Compressor(FS)
    cm.process(x, pars)
    # the state's fixed point is xL: the output level, before the rounding to float, is xG + M - yL
    a = float(x[0, 0])
    return 20.0 * np.log10(a) + pars[3] - cm.yL, 20.0 * np.log10(a), pars


@pytest.mark.parametrize("level_db, params", [(-6.0, {}), (0.0, dict(threshold=-30.0, knee=10.0, ratio=4.0, makeupGain=6.0)),
                                              (-10.0, dict(threshold=-40.0, knee=0.0, ratio=20.0, makeupGain=-3.0))])
def test_steady_state_above_the_knee(level_db, params):
    params = dict(attack=0.001, release=0.005, **params)   # (settles within the 400 blocks)
    out_db, in_db, (T, W, R, Mk, _, _) = _settled_level_db(level_db, **params)
    assert in_db > T + W / 2
    assert abs(out_db - (T + (in_db - T) / R + Mk)) <= 1e-9


def test_below_the_knee_the_output_is_the_input_times_the_makeup_gain_exactly():
    pars = M.block_params(FS, threshold=-20.0, knee=12.0, makeupGain=5.0)
    rng = np.random.default_rng(1)
    x = (rng.uniform(-1, 1, size=(2, 512)) * 10.0 ** (-27.0 / 20.0)).astype(np.float32)   # peaks at -27 dB < T - W/2 = -26 dB
    cm = M.Compressor(FS)
    y = cm.process(x, pars)
    g = np.float32(np.power(10.0, 5.0 / 20.0))
    assert cm.yL == 0.0
    assert np.array_equal(y, x * g)


def test_w_zero_takes_the_hard_knee_branch():
    T, R = -20.0, 4.0
    a = np.array([10.0 ** (-30 / 20.0), 10.0 ** (-20.0001 / 20.0), 10.0 ** (-19.9999 / 20.0), 10.0 ** (-8 / 20.0), 1.0], dtype=np.float32)
    xL = M.level_reduction(a, T, 0.0, R)
    xG = 20.0 * np.log10(a.astype(np.float64))
    assert np.all(np.isfinite(xL))
    assert xL[0] == 0.0 and xL[1] == 0.0
    for k in (2, 3, 4):
        assert xL[k] == xG[k] - (T + (xG[k] - T) / R)   # T + d / R, not the knee's parabola
    assert abs(xL[4] - 15.0) < 1e-12


def test_attack_zero_limits_a_step_in_the_same_frame():
    pars = M.block_params(FS, threshold=-12.0, knee=0.0, ratio=20.0, attack=0.0)
    assert pars[4] == 0.0
    x = np.zeros((1, 256), dtype=np.float32)
    x[0, 100:] = 1.0
    y = M.Compressor(FS).process(x, pars)
    assert np.all(y[0, :100] == 0.0)
    want = np.float32(np.power(10.0, -(0.0 - (-12.0 + 12.0 / 20.0)) / 20.0))   # yL = xL in the step's own frame
    assert y[0, 100] == want and np.all(y[0, 100:] == want)
    assert 20.0 * np.log10(float(want)) == pytest.approx(-11.4, abs=1e-6)


def test_after_the_input_goes_silent_yl_decays_as_ar_to_the_n():
    pars = M.block_params(FS, release=0.05)
    aR = pars[5]
    assert aR == float(np.exp(-1.0 / (float(np.float32(0.05)) * FS)))
    cm = M.Compressor(FS)
    cm.process(np.full((1, 1280), 0.9, dtype=np.float32), pars)
    y0 = cm.yL
    assert y0 > 1.0
    twin = M.Compressor(FS)
    twin.yL = y0
    cm.silence(300, pars)
    twin.process(np.zeros((1, 384), dtype=np.float32)[:, :300], pars)   # zeros through the general path: the same sequence
    want = y0
    for _ in range(300):
        want = aR * want
    assert cm.yL == want == twin.yL
    assert cm.yL == pytest.approx(y0 * aR ** 300, rel=1e-12)


def test_state_carries_across_calls():
    pars = [M.block_params(FS), M.block_params(FS, threshold=-40.0, ratio=3.0), M.block_params(FS, knee=0.0)]
    x = M.bursts(7, 3 * 128, channels=2)
    whole = M.Compressor(FS).process(x, pars)
    cm = M.Compressor(FS)
    parts = [cm.process(x[:, b * 128:(b + 1) * 128], pars[b]) for b in range(3)]
    assert np.array_equal(whole, np.concatenate(parts, axis=1))
