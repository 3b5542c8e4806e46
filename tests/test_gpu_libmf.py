"""graphaudio_amd/csrc/ga_libmf.hpp on the device (option "libm_exact"): tests/libmf_main.hip evaluates ga_cosf /
ga_sinf on about 2^24 arguments and ga_powf(10, .) on about 2^24 exponents in two kernels, the host evaluates the same header on the
same arguments, and the condition is identical bit patterns.  This is the check of the device's double arithmetic and of the
compiler (no contraction, the tables); which libm the machine has plays no part (that is tests/test_libmf_host.py)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "graphaudio_amd", "libmf_check")


@pytest.mark.gpu
def test_device_evaluates_the_header_as_the_host_does():
    assert os.path.isfile(EXE), "graphaudio_amd/libmf_check is missing: the csrc Makefile's `all` target builds it"
    r = subprocess.run(["timeout", "-k", "10", "120", EXE], capture_output=True, text=True)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok")
    rows = {n: (int(c), int(bad)) for n, c, bad in re.findall(r"^(ga_\w+) (\d+) arguments, device != host: (\d+)", r.stdout, re.M)}
    assert sorted(rows) == ["ga_cosf", "ga_powf", "ga_sinf"]
    assert all(bad == 0 for _, bad in rows.values())
    assert rows["ga_cosf"][0] == rows["ga_sinf"][0] == 0x40800000 // 64 + 1 + 2 * (7 * 129 + 65)
    assert rows["ga_powf"][0] == 0x3FC00000 // 64 + 1 + (1 << 20)
