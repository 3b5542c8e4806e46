"""The host arithmetic of the time-split biquad path -- graphaudio_amd/csrc/ga_biquad_split.hpp: the rounding-deviation predictor, A and
A^K, the cut rule -- against tests/biquad_split_ref.hpp, and that reference against itself.

tests/biquad_split_main.cpp is built with g++ under the address and undefined-behaviour sanitizers, with -ffp-contract=off and no
fast-math or flush-to-zero flag, and run directly (no GPU, no HIP), once for all tests of this file:
  transition.s<k>.<family>  A^K (float64, repeated squaring) against K sequential steps of the recurrence in long double, K in
                            {1, 2, 3, 32, 768, 1024, 1056, 16384}, 1..8 sections, inside a bound derived in the program's comments
  split_equals_one_walk     where A^K is exactly zero, the split model and the one walk are the same bits
  deviation.*               270 cascades of 1..3 sections that mode 1 splits: the measured split-vs-one-walk RMS stays below the
                            predicted one (worst 0.863 x) and below the option's value; the split is as close to float64 as the one
                            walk (worst ratio 1.0892, pinned: 1.25 x that is allowed); three cascades outside the threshold, declined
  cut_rule                  pieces are multiples of 32 frames, tile the segment, at most 256
The kernels are held to the same reference, bit for bit, by tests/test_gpu_biquad_split_kernels.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "biquad_split_main.cpp")
TRANSITION = [f"transition.s{k}.{f}" for k in range(1, 9) for f in ("hard", "mid", "mixed")]
DEVIATION = ["deviation.predictor_bounds_the_split", "deviation.split_cascades_stay_inside_the_option",
             "deviation.split_as_close_to_float64_as_one_walk", "deviation.mode1_declines.lowpass_45.7Hz_Q3.95",
             "deviation.mode1_declines.allpass_21Hz_Q1.2_in_3_sections", "deviation.mode1_declines.lowpass_20Hz_Q0.5"]
CHECKS = TRANSITION + ["split_equals_one_walk"] + DEVIATION + ["cut_rule"]


@pytest.fixture(scope="module")
def seen(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("biquad_split") / "biquad_split_san")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "tests"), "-I", os.path.join(ROOT, "graphaudio_amd", "csrc"),
                           SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-8000:], r.stderr[-3000:])
    checks = {}
    for line in r.stdout.splitlines():
        p = line.split()
        if len(p) >= 3 and p[0] == "check":
            checks[p[1]] = p[2]
    assert sorted(checks) == sorted(CHECKS)
    assert r.returncode == (0 if all(v == "ok" for v in checks.values()) else 1), r.returncode   # (anything else: a sanitizer report)
    return checks


def _all_ok(seen, names):
    assert {k: seen[k] for k in names if seen[k] != "ok"} == {}


def test_transition_matrix_inside_the_derived_bound(seen):
    _all_ok(seen, TRANSITION)


def test_split_equals_the_one_walk_where_nothing_crosses_a_piece(seen):
    _all_ok(seen, ["split_equals_one_walk"])


def test_deviation_predictor_bounds_what_mode_1_splits(seen):
    _all_ok(seen, DEVIATION)


def test_cut_rule(seen):
    _all_ok(seen, ["cut_rule"])
