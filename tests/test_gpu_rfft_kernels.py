"""The seven 256-point real-FFT kernels of the convolver path (graphaudio_amd/csrc/ga_rfft.hip), bit for bit.

tests/rfft_kernels_main.hip drives them through their launchers alone, on inputs from a seeded integer generator, at the block
counts, row counts and partition counts where their tiling changes path, and prints one FNV-1a digest per output array.  The
digests in tests/golden/rfft_kernel_digests.json were recorded while every kernel still carried its own copy of the transform;
the bodies are one core now (irfft_ola_b_kernel alone keeps its statements inline), and this test holds them to the values the copies gave.  The program also compares, element
by element, formulation A against B<double> (forward and inverse) and the conv_migrate rebuild against B<double>: all of these
identities held when the digests were recorded."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "graphaudio_amd", "rfft_kernels_check")
GOLDEN = os.path.join(ROOT, "tests", "golden", "rfft_kernel_digests.json")


@pytest.mark.gpu
def test_rfft_kernels_reproduce_the_recorded_digests_and_identities():
    assert os.path.isfile(EXE), "graphaudio_amd/rfft_kernels_check is missing: the csrc Makefile's `all` target builds it"
    with open(GOLDEN, encoding="utf-8") as f:
        golden = json.load(f)
    r = subprocess.run(["timeout", "-k", "10", "120", EXE], capture_output=True, text=True)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0
    digests, identities = {}, {}
    for line in r.stdout.splitlines():
        p = line.split()
        if p and p[0] == "digest":
            digests[p[1]] = p[2]
        elif p and p[0] == "identity":
            identities[p[1]] = p[2]
    assert sorted(digests) == sorted(golden["digests"])
    wrong = [k for k, v in golden["digests"].items() if digests[k] != v]
    assert not wrong, f"{len(wrong)} of {len(digests)} digests differ: {wrong[:8]}"
    assert sorted(identities) == sorted(golden["identities"])
    broken = [k for k, v in identities.items() if v != "ok"]
    assert not broken, broken
