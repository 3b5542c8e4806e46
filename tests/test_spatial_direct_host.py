"""The shared occlusion / transmission statements (graphaudio_amd/csrc/ga_spatial_direct.hpp) built with a plain host compiler, twice:
with the project's flags (-ffp-contract=off, as the library's host and device code are built) and with contraction allowed and fused
multiply-adds available -- the header switches contraction off itself, so both instantiations give the same bits -- against the
float32 restatement and the float64 walk of tests/_spatial_direct_model.py.

Bounds: the occlusion arithmetic is bit for bit.  The float32 sample walk stays within 1e-6 x max(1, peak) of the float64 model: a
one-pole section in transposed direct form II accumulates about |a1| / (1 - |a1|) half-ulps of its output, ~10 x 6e-8 for the 800 Hz
low-pass at 48 kHz; 2e-7 was measured when the order of the band filters was chosen.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import _spatial_direct_model as DM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphaudio_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "spatial_direct_main.cpp")
SR = 48000
B = 128
f32 = np.float32


def cpu_has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return any(line.startswith("flags") and " fma" in line for line in f)
    except OSError:
        return False


FLAGS = {"project": ["-O1", "-ffp-contract=off"],
         "contracting": ["-O3", "-ffp-contract=fast"] + (["-mfma"] if cpu_has_fma() else [])}


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("spatial_direct")
    exes = {}
    for name, flags in FLAGS.items():
        exes[name] = str(d / name)
        subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-I", CSRC, MAIN, "-o", exes[name]])
    return exes


def run(exe, args, data):
    got = subprocess.run([exe, *args], input=np.asarray(data, np.float32).tobytes(), capture_output=True, check=True).stdout
    return np.frombuffer(got, np.float32)


def occlusion_grid():
    rng = np.random.default_rng(7)
    occs = [0.0, 1.0, float(np.nextafter(f32(0), f32(1))), 1e-6, 0.25, 0.6, 0.999, -0.5]
    ts = [(0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.4, 0.4, 0.4), (0.9, 0.5, 0.1), (0.1, 0.5, 0.9), (0.0, 1.0, 0.0), (0.3, 0.0, 0.0), (0.0, 0.0, 1e-3)]
    grid = [(o, *t) for o in occs for t in ts]
    grid += [tuple(float(v) for v in rng.uniform(0.0, 1.0, 4)) for _ in range(200)]
    return np.asarray(grid, np.float32)


def test_occlusion_arithmetic_is_bit_equal_in_both_instantiations(programs):
    grid = occlusion_grid()
    got = {name: run(exe, ["occ"], grid).reshape(-1, 4) for name, exe in programs.items()}
    want = np.asarray([[s, *c] for s, c in (DM.occlusion(*row) for row in grid)], np.float32)
    for name, g in got.items():
        assert g.shape == want.shape
        assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), name
    # what the grid is there for: open air is the identity, equal transmission is a plain gain, all-zero transmission is 1 - occ
    for row, (s, cm, cl, ch) in zip(grid, want):
        occ, tl, tm, th = row
        if occ <= 0:
            assert (s, cm, cl, ch) == (1, 1, 0, 0), row
        elif tl == tm == th:
            assert (cm, cl, ch) == (1, 0, 0) or s == 0, row
            if tl == 0:
                assert s == f32(f32(1) - occ), row
    assert any(r[0] == 1 and not r[1:].any() for r in grid) and any(0 < r[0] < 1e-30 for r in grid)
    fully = want[[i for i, r in enumerate(grid) if r[0] == 1 and not r[1:].any()][0]]
    assert tuple(fully) == (0, 1, 0, 0)          # fully blocked, nothing passes: s = 0, the EQ stays the identity


def walk_inputs():
    rng = np.random.default_rng(11)
    nb = 48
    t = np.arange(nb * B) / SR
    signals = {"noise": (rng.standard_normal(nb * B) * 0.3).astype(np.float32), "sine 30 Hz": np.sin(2 * np.pi * 30.0 * t).astype(np.float32)}
    triples = []
    for b in range(nb):     # a triple that changes every block, with stretches of identity: two runs, ramp-in and ramp-out blocks
        if b in (0, 1, 20, 21, 22, 23):
            triples.append(DM.EQ_IDENTITY)
        else:
            triples.append(DM.occlusion(*rng.uniform(0.05, 1.0, 4))[1])
    return nb, signals, np.asarray(triples, np.float32)


def test_sample_walk_against_the_float64_model(programs):
    nb, signals, triples = walk_inputs()
    assert sum(1 for t in triples if tuple(t) != DM.EQ_IDENTITY) >= 40
    for what, x in signals.items():
        ref = DM.direct(x, triples, sample_rate=SR)[0]
        outs = {name: run(exe, ["walk", str(SR), str(nb)], np.concatenate([triples.ravel(), x])) for name, exe in programs.items()}
        assert np.array_equal(outs["project"].view(np.uint32), outs["contracting"].view(np.uint32)), what
        scale = max(1.0, float(np.max(np.abs(ref))))
        err = float(np.max(np.abs(outs["project"].astype(np.float64) - ref)))
        print(f"{what}: max-abs error {err:.3e} = {err / scale:.3e} x max(1, peak {float(np.max(np.abs(ref))):.3f})")
        assert float(np.max(np.abs(ref - x))) > 1e-2          # the stage is heard
        assert err <= 1e-6 * scale, (what, err)
        for b in (0, 22, 23):                                 # neither triple differs from the identity: x itself
            assert np.array_equal(outs["project"][b * B:(b + 1) * B].view(np.uint32), x[b * B:(b + 1) * B].view(np.uint32)), (what, b)


def test_identity_triple_is_bit_for_bit(programs):
    nb = 6
    x = (np.random.default_rng(3).standard_normal(nb * B) * 0.7).astype(np.float32)
    x[5] = -0.0
    triples = np.asarray([DM.EQ_IDENTITY] * nb, np.float32)
    for name, exe in programs.items():
        out = run(exe, ["walk", str(SR), str(nb)], np.concatenate([triples.ravel(), x]))
        assert np.array_equal(out.view(np.uint32), x.view(np.uint32)), name
