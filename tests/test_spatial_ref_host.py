"""tests/spatial_ref.hpp, the reference of the SpatialPannerNode kernels (graphaudio_amd/csrc/ga_spatial.hip), against itself.

tests/spatial_ref_main.cpp is built with g++ under the address and undefined-behaviour sanitizers, with -ffp-contract=off, and run
directly (no GPU, no HIP): the float64 form against a naive double loop written on its own (1e-12 relative) and against
tests/_spatial_model.render on the recorded case tests/golden/spatial_ref_case.bin (tests/golden/make_spatial_ref_case.py), the
float32 chain within its derived bound of the float64 form and equal to it on the exact scenes, a chunk cut at every block in both
forms, the work lists and the table check, and the occlusion walk cut in two.  The kernels are held to this reference by
tests/test_gpu_spatial_kernels.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "spatial_ref_main.cpp")
CASE = os.path.join(ROOT, "tests", "golden", "spatial_ref_case.bin")
CHECKS = ["a_vs_naive", "a_vs_model", "b_within_bound", "b_exact", "chunk_cut_a", "chunk_cut_b", "works", "direct_walk_cut"]


def test_reference_against_itself_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "spatial_ref_san")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "tests"),
                           "-I", os.path.join(ROOT, "graphaudio_amd", "csrc"), SRC, "-o", exe])
    r = subprocess.run([exe, CASE], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-3000:])
    assert r.returncode == 0
    seen = {}
    for line in r.stdout.splitlines():
        p = line.split()
        if p and p[0] == "check":
            seen[p[1]] = p[2]
    assert sorted(seen) == sorted(CHECKS)
    assert all(v == "ok" for v in seen.values()), seen
