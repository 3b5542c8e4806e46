"""tests/coarse_ref.hpp, the float64 reference of the coarse convolver kernels (graphaudio_amd/csrc/ga_coarse.hip), against itself.

tests/coarse_ref_main.cpp is built with g++ under the address and undefined-behaviour sanitizers and run directly (no GPU, no HIP):
the fast transform inside ref_spectrum against a naive O(N^2) DFT of one full window, and ref_inv(ref_mac(ref_fwd(x), ref_fwd(h)))
against direct float64 convolution for a 3-partition response and a 5-block signal with history, to 1e-12 relative.  The kernels are
held to this reference by tests/test_gpu_coarse_kernels.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "coarse_ref_main.cpp")
CHECKS = ["spectrum_vs_naive_dft", "chain_vs_direct_convolution"]


def test_reference_against_itself_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "coarse_ref_san")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O2", "-g", "-fsanitize=address,undefined",
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
