"""tests/rfft_ref.hpp, the float64 reference of the 256-point real-FFT kernels (graphaudio_amd/csrc/ga_rfft.hip), against itself.

tests/rfft_ref_main.cpp is built with g++ under the address and undefined-behaviour sanitizers, with -ffp-contract=off, and run
directly (no GPU, no HIP): the radix-2 forward and inverse transforms against the O(N^2) sums the contract is written as (1e-12
relative), inverse(forward(x)) = [x | 0], the overlap-add of inverse(forward(x) H) over several blocks against direct linear
convolution with a 129-tap filter (1e-12), and the two plane layouts.  The kernels are held to this reference by
tests/test_gpu_rfft_ref.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "rfft_ref_main.cpp")
CHECKS = ["forward_vs_naive", "inverse_vs_naive", "roundtrip", "ola_vs_linear_convolution", "layouts"]


def test_reference_against_itself_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "rfft_ref_san")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "tests"), SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-3000:])
    assert r.returncode == 0
    seen = {}
    for line in r.stdout.splitlines():
        p = line.split()
        if p and p[0] == "check":
            seen[p[1]] = p[2]
    assert sorted(seen) == sorted(CHECKS)
    assert all(v == "ok" for v in seen.values()), seen
