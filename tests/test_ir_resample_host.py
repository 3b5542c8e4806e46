"""Option "ir_resample" ("Impulse responses at another sample rate"), the parts that need no GPU:
graphaudio_amd/csrc/ga_ir_resample.hpp, run by tests/ir_resample_main.cpp, against the float64 model tests/_ir_resample_model.py.

The condition is |got - model| <= 2^-23 |model| + 1e-12 for inputs in [-1, 1].  It is derived, not measured: one float rounding (2^-24
relative) with a factor 2 for values the two evaluations round across a boundary, plus the error of a double sum of at most 3,270
terms with sum |x h| < 10 (3,270 x 2^-53 x 10 < 4e-12 in the worst case, a few 1e-14 for rounding errors of random sign)."""
import os
import subprocess

import numpy as np
import pytest

from tests import _ir_resample_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ir_resample_main.cpp")
INC = os.path.join(ROOT, "graphaudio_amd", "csrc")

# (fi, fo, L, D, W)
PAIRS = [(44100, 48000, 160, 147, 69), (48000, 44100, 147, 160, 75), (96000, 48000, 1, 2, 137), (8000, 48000, 6, 1, 69),
         (192000, 8000, 1, 24, 1635)]


def _read(*parts):
    with open(os.path.join(ROOT, *parts), encoding="utf-8") as f:
        return f.read()


def _build(tmp_path, name, *flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", INC, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("ir_resample"), "ir_resample_main", "-O2")


def _lengths(W):
    return [1, 2, W, 2 * W - 1, 2 * W, 2 * W + 1, 700]


def _rows(fi, fo, n):
    rng = np.random.default_rng(fi * 7 + fo * 3 + n)
    x = rng.uniform(-1.0, 1.0, size=(2, n)).astype(np.float32)
    x[0, 0] = 1.0
    x[1, -1] = -1.0
    return x


def _run(program, tmp_path, x, fi, fo):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    x.astype(np.float32).tofile(src)
    r = subprocess.run([program, "run", str(fi), str(fo), str(x.shape[0]), str(x.shape[1]), str(src), str(dst)], capture_output=True, text=True)
    print(r.stdout[-1000:], r.stderr[-2000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok")
    return np.fromfile(dst, dtype=np.float32).reshape(x.shape[0], -1), r.stdout


def _check(got, want):
    assert got.shape == want.shape
    err = np.abs(got.astype(np.float64) - want)
    bound = 2.0 ** -23 * np.abs(want) + 1e-12
    print(f"max error / bound {float(np.max(err / bound)):.3f}")
    assert np.all(err <= bound)


@pytest.mark.parametrize("fi,fo,L,D,W", PAIRS, ids=lambda v: str(v))
def test_header_against_the_model(program, tmp_path, fi, fo, L, D, W):
    p = model.plan(fi, fo)
    assert (p.L, p.D, p.W) == (L, D, W)
    for n in _lengths(W):
        x = _rows(fi, fo, n)
        got, out = _run(program, tmp_path, x, fi, fo)
        m = (n * L + D - 1) // D
        assert f"plan {L} {D} {W} {L * 2 * W}" in out and f"M {m}" in out
        assert got.shape[1] == m
        _check(got, model.resample(x, fi, fo))


def test_a_delta_stays_a_band_limited_identity(program, tmp_path):
    fi, fo = 44100, 48000
    x = np.zeros((1, 400), dtype=np.float32)
    x[0, 200] = 1.0
    got, _ = _run(program, tmp_path, x, fi, fo)
    y = got[0].astype(np.float64)
    assert y.size == (400 * 160 + 146) // 147
    assert abs(np.sum(y) - 1.0) <= 1e-6
    t = np.arange(y.size) / fo

    def response(f):
        return abs(np.sum(y * np.exp(-2j * np.pi * f * t)))

    print(f"sum {np.sum(y):.9f}  |H(1 kHz)| {response(1000.0):.9f}  |H(22050 Hz)| {response(22050.0):.3e}")
    assert abs(response(1000.0) - 1.0) <= 1e-5
    assert response(22050.0) < 1e-5


def test_the_plan_refuses_a_table_beyond_the_cap(program):
    assert model.plan(44101, 48000) is None and 48000 * 2 * 69 == 6624000 > 1 << 22
    r = subprocess.run([program, "plan", "44101", "48000"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["refused", "ok"]
    r = subprocess.run([program, "plan", "11025", "192000"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split()[:5] == ["plan", "2560", "147", "69", "353280"]


def test_header_under_the_sanitizers(tmp_path):
    exe = _build(tmp_path, "ir_resample_san", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
    for fi, fo, L, D, W in PAIRS:
        for n in _lengths(W):
            x = _rows(fi, fo, n)
            got, _ = _run(exe, tmp_path, x, fi, fo)
            _check(got, model.resample(x, fi, fo))


def test_the_option_is_named_where_a_host_looks_for_it():
    assert '"ir_resample"' in _read("include", "graphaudio_hip.h")
    cs = _read("bindings", "csharp", "HipOfflineAudioContext.cs")
    assert "public bool IrResample" in cs and '"ir_resample"' in cs
    assert "ir_resample" in _read("INTEGRATION.md")
    assert "ir_resample" in _read("DESIGN.md")
    assert "ir_resample" in _read("README.md")


def test_ir_resamples_is_in_the_statistics_of_all_three_declarations():
    from graphaudio_amd import _capi
    names = [n for n, _ in _capi.Stats._fields_]
    assert "ir_resamples" in names
    header = _read("include", "graphaudio_hip.h")
    body = header[header.index("typedef struct ga_stats"):header.index("} ga_stats;")]
    assert "int64_t ir_resamples;" in body
    cs = _read("bindings", "csharp", "GraphAudioHip.cs")
    stats = cs[cs.index("public unsafe struct Stats"):]
    assert "public long ir_resamples;" in stats[:stats.index("}")]
    # the same neighbours in all three: behind delay_flags_predicted
    assert names[names.index("ir_resamples") - 1] == "delay_flags_predicted"
    assert body.index("delay_flags_predicted") < body.index("ir_resamples;") < body.index("conv_migrations;")
