"""ir_resample_kernel on the device (option "ir_resample", DESIGN.md section 8 "Impulse responses at another sample rate"):
tests/ir_resample_main.hip runs the kernel through launch_ir_resample, the launcher the library uses, and the host evaluates the
same header (graphaudio_amd/csrc/ga_ir_resample.hpp) on the same rows and the same table.  The condition is identical bit patterns.

Per rate pair: N = 1, 2, 2W-1, 2W, 2W+1; M = tile - 1, tile, tile + 1, 3 tiles + 5; 1, 3 and 4096 channels; rows N + 1 floats apart
and one float off the allocation, so no row is aligned; -0.0f, denormals and +-1 among the inputs.  The floats behind every output
row must keep their fill pattern (they count as differences)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "graphaudio_amd", "ir_resample_check")

PAIRS = {"44100-48000": (160, 147, 69), "48000-44100": (147, 160, 75), "96000-48000": (1, 2, 137), "8000-48000": (6, 1, 69),
         "192000-8000": (1, 24, 1635)}
SHAPES = ["N=1/ch=3", "N=2/ch=3", "N=2W-1/ch=3", "N=2W/ch=3", "N=2W+1/ch=3", "M=tile-1/ch=3", "M=tile/ch=3", "M=tile+1/ch=3",
          "M=3tiles+5/ch=3", "N=2W+1/ch=1", "N=16/ch=4096"]


def _m(n, L, D):
    return (n * L + D - 1) // D


@pytest.mark.gpu
def test_device_evaluates_the_header_as_the_host_does():
    assert os.path.isfile(EXE), "graphaudio_amd/ir_resample_check is missing: the csrc Makefile's `all` target builds it"
    r = subprocess.run(["timeout", "-k", "10", "120", EXE], capture_output=True, text=True)
    print(r.stdout[-8000:], r.stderr[-2000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok")
    plans = {n: (int(L), int(D), int(W), int(t)) for n, L, D, W, t in re.findall(r"^pair (\S+) L (\d+) D (\d+) W (\d+) tile (\d+)", r.stdout, re.M)}
    assert {n: p[:3] for n, p in plans.items()} == PAIRS
    rows = re.findall(r"^(\S+) (\d+) outputs, device != host: (\d+)", r.stdout, re.M)
    assert [n for n, _, _ in rows] == [f"{p}/{s}" for p in PAIRS for s in SHAPES]
    assert all(int(bad) == 0 for _, _, bad in rows)
    count = {n: int(c) for n, c, _ in rows}
    for p, (L, D, W, tile) in plans.items():
        assert 1 <= tile <= 256
        for name, n in (("N=1", 1), ("N=2", 2), ("N=2W-1", 2 * W - 1), ("N=2W", 2 * W), ("N=2W+1", 2 * W + 1)):
            assert count[f"{p}/{name}/ch=3"] == 3 * _m(n, L, D)
        assert count[f"{p}/N=2W+1/ch=1"] == _m(2 * W + 1, L, D)
        assert count[f"{p}/N=16/ch=4096"] == 4096 * _m(16, L, D)
        step = max(1, -(-L // D))   # consecutive N move M by at most this: how far upsampling can miss a target
        for name, target, below in (("M=tile-1", max(tile - 1, 1), True), ("M=tile", tile, False), ("M=tile+1", tile + 1, False),
                                    ("M=3tiles+5", 3 * tile + 5, False)):
            m, rem = divmod(count[f"{p}/{name}/ch=3"], 3)
            assert rem == 0 and (target - step < m <= target if below else target <= m < target + step), (p, name, m, target)
        # every case of more than one tile exists for every pair
        assert count[f"{p}/M=3tiles+5/ch=3"] // 3 > 3 * tile
