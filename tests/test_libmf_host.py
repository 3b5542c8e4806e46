"""Option "libm_exact" (libm class), the parts that need no GPU: graphaudio_amd/csrc/ga_libmf.hpp restates
glibc's cosf / sinf / powf, and tests/libmf_main.cpp compares it bit pattern by bit pattern with the C library of the machine the
test runs on.  Zero mismatches is the condition: it says both that the restatement is right and that this machine's libm is of the
family the option is for (on a host with another libm the option stays off)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "libmf_main.cpp")
INC = os.path.join(ROOT, "graphaudio_amd", "csrc")


def _read(*parts):
    with open(os.path.join(ROOT, *parts), encoding="utf-8") as f:
        return f.read()


def _build(tmp_path, name, *flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-pthread", *flags, "-I", INC, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("libmf"), "libmf_main", "-O2")


def test_the_option_is_named_where_a_host_looks_for_it():
    assert '"libm_exact"' in _read("include", "graphaudio_hip.h")
    cs = _read("bindings", "csharp", "HipOfflineAudioContext.cs")
    assert "public bool LibmExact" in cs and '"libm_exact"' in cs
    assert "libm_exact" in _read("INTEGRATION.md")
    assert "libm_exact" in _read("DESIGN.md")
    assert "libm_exact" in _read("README.md")


def test_restatement_equals_the_c_library_on_the_quick_sweep(program):
    r = subprocess.run([program, "quick"], capture_output=True, text=True)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok")
    rows = re.findall(r"^(\S.*?)\s+(\d+) arguments, restatement != libm: (\d+)", r.stdout, re.M)
    assert [n for n, _, _ in rows] == ["sinf", "cosf", "sinf edges", "cosf edges", "powf(10.0)", "powf gains"]
    assert all(int(bad) == 0 for _, _, bad in rows)
    count = {n: int(c) for n, c, _ in rows}
    # every 16th float of [0, 4.0] and of [0, 1.5], both signs; 8 neighbourhoods of up to 129 floats, both signs; 2^20 gains
    assert count["sinf"] == count["cosf"] == 2 * (0x40800000 // 16 + 1) and count["powf(10.0)"] == 2 * (0x3FC00000 // 16 + 1)
    assert count["sinf edges"] == count["cosf edges"] == 2 * (7 * 129 + 65) and count["powf gains"] == 1 << 20


def test_gains_mode_finds_the_gains_of_the_pow_scene(program):
    """tests/test_gpu_libm_exact.py steps a k-rate gain through gains at which powf(10, g / 40) is not the rounded-once double: the
    ones this mode prints on a glibc host.  Here: the list is reproduced, and the restatement is powf's value at each of them."""
    from tests._libm_scenes import POW_GAIN_BITS
    r = subprocess.run([program, "gains"], capture_output=True, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0
    rows = re.findall(r"^gain \S+ bits 0x([0-9a-f]{8}) powf 0x([0-9a-f]{8}) rounded-once 0x([0-9a-f]{8}) restated 0x([0-9a-f]{8})", r.stdout, re.M)
    assert len(rows) == 32
    assert all(p == m and p != o for _, p, o, m in rows)
    printed = [int(g, 16) for g, _, _, _ in rows]
    assert all(b in printed for b in POW_GAIN_BITS) and len(set(POW_GAIN_BITS)) == 24


def test_header_under_the_sanitizers(tmp_path):
    exe = _build(tmp_path, "libmf_san", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
    for mode in ("quick", "gains"):
        r = subprocess.run([exe, mode], capture_output=True, text=True)
        print(r.stdout[-2000:], r.stderr[-2000:])
        assert r.returncode == 0 and r.stdout.strip().endswith("ok")
