"""compressor_kernel alone (graphaudio_amd/csrc/ga_dynamics.hip; DynamicsCompressorNode):
tests/compressor_main.hip runs the kernel through launch_compressor, the launcher the library uses, on a case this file writes, and
the outputs are compared with the float64 model of tests/_compressor_model.py.

Three nodes in every launch, each with its own parameters, which change at block 2:
  node 0  mono, one silent block (block 3: only yL moves); W = 0 in blocks 0-1
  node 1  stereo; attack = 0 throughout, release = 0 from block 2 on
  node 2  one channel in blocks 0-2, two from block 3 on (a segment boundary inside the job); R = 1 in blocks 0-1, then
          threshold -100 with knee 40, where T - W/2 is the -120 dB floor of the level
Input: seeded noise bursts at -40, -12 and 0 dBFS with silent gaps.  Lengths 1, 2 and 5 blocks (one tile pair, a block boundary, an
odd count).  The 5 blocks as one launch, as 2 + 3 and as 1 x 5 with yL carried in device memory must be bit-identical.

Truth: every sample within 2^-22 |m| of the model m -- two float ulps: the device's and numpy's double log10 / pow agree to about
1e-15 relative, so g differs by at most one float ulp after its rounding and the product adds half an ulp; a branch flip at
xL ~ yLprev is harmless because the branches meet there.  No sample is left out; where the model is exactly 0 the sample is
exactly 0.  What the kernel must not write (silent blocks, channel 1 of mono blocks, blocks behind the rendered ones) keeps the fill."""
import os
import subprocess

import numpy as np
import pytest

from tests import _compressor_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "graphaudio_amd", "compressor_check")
FS = 48000
BLOCKS = 5
FRAMES = BLOCKS * 128
FILL = 0xCDCDCDCD
SPLITS = ["1", "2", "5", "2,3", "1,1,1,1,1"]

NCH = [[1, 1, 1, 0, 1], [2, 2, 2, 2, 2], [1, 1, 1, 2, 2]]
PARAMS = [   # per node: blocks 0-1, blocks 2-4
    (dict(threshold=-30.0, knee=0.0, ratio=4.0, attack=0.003, release=0.05, makeupGain=3.0),
     dict(threshold=-20.0, knee=6.0, ratio=8.0, attack=0.003, release=0.01, makeupGain=0.0)),
    (dict(attack=0.0),
     dict(threshold=-50.0, knee=40.0, ratio=20.0, attack=0.0, release=0.0, makeupGain=-6.0)),
    (dict(ratio=1.0, makeupGain=0.0),
     dict(threshold=-100.0, knee=40.0, ratio=2.0, attack=0.0005, release=0.25, makeupGain=12.0)),
]


def _values(p):
    return [np.float32(min(max(np.float32(p.get(name, default)), np.float32(mn)), np.float32(mx))) for name, default, mn, mx in M.PARAMS]


def _case():
    orders = [(-12.0, -40.0, 0.0), (-40.0, -12.0, 0.0), (0.0, -40.0, -12.0)]   # (node 0 is above its hard knee within blocks 0-1)
    xs = [M.bursts(100 + k, FRAMES, channels=2, levels_db=orders[k]) for k in range(3)]
    xs[0][1] = 0.0   # (channels a node does not have are not read)
    xs[2][1, :3 * 128] = 0.0
    return xs


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    assert os.path.isfile(EXE), "graphaudio_amd/compressor_check is missing: the csrc Makefile's `all` target builds it"
    d = tmp_path_factory.mktemp("compressor")
    xs = _case()
    with open(d / "case.bin", "wb") as f:
        f.write(np.array([3, BLOCKS], dtype=np.int32).tobytes())
        for k in range(3):
            f.write(np.array(NCH[k], dtype=np.int32).tobytes())
            f.write(np.array([_values(PARAMS[k][0 if b < 2 else 1]) for b in range(BLOCKS)], dtype=np.float32).tobytes())
            f.write(np.ascontiguousarray(xs[k], dtype=np.float32).tobytes())
    out = {}
    for sp in SPLITS:
        path = d / ("out_" + sp.replace(",", "_") + ".bin")
        r = subprocess.run(["timeout", "-k", "10", "60", EXE, str(d / "case.bin"), str(path), sp], capture_output=True, text=True)
        print(sp, r.stdout[-2000:], r.stderr[-2000:])
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), sp
        raw = open(path, "rb").read()
        y = np.frombuffer(raw[:3 * 2 * FRAMES * 4], dtype=np.float32).reshape(3, 2, FRAMES)
        yl = np.frombuffer(raw[3 * 2 * FRAMES * 4:], dtype=np.float64)
        out[sp] = (y, yl)
    return xs, out


def _model(xs, k, nblocks):
    """node k over the first nblocks blocks: (y [2][frames] with NaN where nothing may be written, final yL)"""
    cm = M.Compressor(FS)
    y = np.full((2, FRAMES), np.nan)
    for b in range(nblocks):
        pars = M.block_params(FS, **PARAMS[k][0 if b < 2 else 1])
        sl = slice(b * 128, (b + 1) * 128)
        if NCH[k][b] == 0:
            cm.silence(128, pars)
        else:
            y[:NCH[k][b], sl] = cm.process(xs[k][:NCH[k][b], sl], pars)
    return y, cm.yL


@pytest.mark.gpu
@pytest.mark.parametrize("split", SPLITS)
def test_every_sample_is_within_two_ulps_of_the_model(runs, split):
    xs, out = runs
    y, yl = out[split]
    nblocks = sum(int(v) for v in split.split(","))
    for k in range(3):
        m, m_yl = _model(xs, k, nblocks)
        written = ~np.isnan(m)
        bits = y[k].view(np.uint32)
        assert np.all(bits[~written] == FILL), (split, k, "wrote where it must not")
        print(f"split {split} node {k}: worst |y - m| / |m| = {M.worst(y[k][written], m[written]):.3e} (bound {M.TOL:.3e}), "
              f"yL device {yl[k]!r} model {m_yl!r}")
        assert np.any(m[written] != 0)
        assert M.within(y[k][written], m[written]), (split, k)
        assert abs(yl[k] - m_yl) <= 1e-12, (split, k)   # dB: log10 / pow agree to ~1e-15, and the recurrence is a convex combination


def test_the_cases_reach_every_branch():
    xs = _case()
    seen = set()
    for k in range(3):
        for b in range(BLOCKS):
            if NCH[k][b] == 0:
                continue
            T, W, R, _, aA, aR = M.block_params(FS, **PARAMS[k][0 if b < 2 else 1])
            a = np.max(np.abs(xs[k][:NCH[k][b], b * 128:(b + 1) * 128]), axis=0).astype(np.float64)
            d = 20.0 * np.log10(np.maximum(a, 1e-6)) - T
            seen |= {"below"} if np.any(2 * d < -W) else set()
            seen |= {"knee"} if W > 0 and np.any(np.abs(2 * d) <= W) else set()
            seen |= {"above"} if np.any(2 * d > W) else set()
            seen |= {"hard"} if W == 0 and np.any(2 * d >= 0) else set()
            seen |= {"attack0"} if aA == 0 else set()
            seen |= {"release0"} if aR == 0 else set()
            seen |= {"ratio1"} if R == 1 else set()
    assert seen == {"below", "knee", "above", "hard", "attack0", "release0", "ratio1"}


@pytest.mark.gpu
def test_split_renders_are_bit_identical(runs):
    _, out = runs
    whole = out["5"]
    for sp in ("2,3", "1,1,1,1,1"):
        assert np.array_equal(whole[0].view(np.uint32), out[sp][0].view(np.uint32)), sp
        assert np.array_equal(whole[1].view(np.uint64), out[sp][1].view(np.uint64)), sp
