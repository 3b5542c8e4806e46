"""tests/conv_ref.hpp, the reference of the fine-partition convolver kernels (formulations A, B, R and C, the taps' spectra and the plane
utilities of graphaudio_amd/csrc/ga_conv.hip), against itself.

tests/conv_ref_main.cpp is built with g++ under the address and undefined-behaviour sanitizers, with -ffp-contract=off and no
fast-math or flush-to-zero flag, and run directly (no GPU, no HIP): the fast float64 transform against a naive O(N^2) DFT, the float64
sums against direct summation and against overlap-save through the transforms (1e-12 relative), the float32 reference-order loop of
formulation R against a second, independently written scalar loop bit for bit (uniform inputs, subnormal products, no history), and
the utilities.  The kernels are held to this reference by tests/test_gpu_conv_kernels.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "conv_ref_main.cpp")
CHECKS = ["spectrum_vs_naive_dft", "linconv_vs_direct_summation", "mac_a_vs_direct_summation", "overlap_save_vs_linconv",
          "refmac_vs_second_loop.uniform", "refmac_vs_second_loop.subnormal", "refmac_vs_second_loop.nohist", "utilities"]


def test_reference_against_itself_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "conv_ref_san")
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
