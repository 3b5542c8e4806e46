"""The fine-partition convolver kernels of graphaudio_amd/csrc/ga_conv.hip alone -- formulations A, B, R and C, the taps' spectra
and the five plane utilities -- against the reference tests/conv_ref.hpp.

tests/conv_kernels_main.hip drives them through their launchers on plain device tables, one family per process run, and prints one
line per check ("check <name> ok|FAIL <figures>") and one line per launch of a templated kernel with the name of the instance the
launcher ran.  Here every check must say ok, the set of check names must be the one listed below (a case that was silently skipped
fails), and the set of instance names must be the six tconv / tconv16 instances and the three tap_spectra instances (nine in all).  Families a, b
and util are exact; r_int is exact on integer spectra and r_f32 equal to the float32 reference-order loop bit for bit on uniform ones,
both on every shape of b; tap and c
assert bounds derived in the program's comments ("The fine-partition kernels alone").  If a family ends on a
signal, its time limit or a HIP error (exit status 3), the families behind it are skipped: nothing more is started on a GPU that has just faulted."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "graphaudio_amd", "conv_kernels_check")

LENGTHS = (1024, 2048, 4096)
TAP_INSTANCES = [f"tap_spectra_kernel<{n}>" for n in LENGTHS]
C_INSTANCES = [f"{k}<{n}>" for k in ("tconv_kernel", "tconv16_kernel") for n in LENGTHS]

P_B = (1, 3, 4, 5, 255, 256, 257, 600)
N_B = (1, 3, 255, 256, 257, 520)


def _r_cases(mode):   # all 80 shapes of b, the second tap segment, the second time tile, and both at once
    return (
        [f"r.{mode}.P{P}.n{n}.hr" for P in P_B for n in N_B]
        + [f"r.{mode}.P{P}.n{n}.h{h}" for P in P_B for n in (3, 257) for h in "0g"]
        + [f"r.{mode}.P{P}.n5.hr" for P in (1023, 1024, 1025, 1030)]
        + [f"r.{mode}.P5.n{n}.hr" for n in (1023, 1024, 1025, 1028)]
        + [f"r.{mode}.P257.n1025.hr", f"r.{mode}.P1030.n1028.hr"]
    )


CHECKS = {
    "a": (
        [f"a.rp{256 if r > 128 else 128}.r{r}.n{n}.P{P}" for P in (1, 2, 15, 16, 17, 64, 65) for n in (1, 63, 64, 65, 130) for r in (1, 128, 129)]
        + [f"a.rp256.r1.n{n}.P17" for n in (1, 65)]
        + [f"a.rp128.r{3 if n == 130 else 1}.n{n}.P{P}" for P in (1024, 1025) for n in (1, 65, 130)]
    ),
    "b": [f"b.P{P}.n{n}.hr" for P in P_B for n in N_B] + [f"b.P{P}.n{n}.h{h}" for P in P_B for n in (3, 257) for h in "0g"],
    "r_int": _r_cases("int"),
    "r_f32": _r_cases("f32") + ["r.tiny.P257.n257.hr"],
    "tap": [f"tap.N{n}.P{P}.c{c}" for n in LENGTHS for P in (1, 65, n // 4, n // 4 + 1) for c in (1, 3)],
    "c": (
        [f"c.1024.{s}.{r}" for s in ("P65.s1", "P65.s2", "P257.s2", "P257.s5") for r in ("r8", "r16")]
        + ["c.1024.tbase.r16", "c.1024.hist0.r8", "c.1024.hist0.r16_refused"]
        + [f"c.2048.{s}.{r}" for s in ("P129.s2", "P512.s1") for r in ("r8", "r16")]
        + ["c.2048.tbase.r16"]
        + [f"c.4096.{s}.{r}" for s in ("P512.s2", "P1024.s1") for r in ("r8", "r16")]
        + ["c.4096.tbase.r16", "c.mixed.r16.launch0", "c.mixed.r16.launch1", "c.mixed.r16.once"]
    ),
    "util": (
        ["util.hist_copy_b", "util.plane_copy.offset", "util.plane_copy.null", "util.plane_copy.strided", "util.extract_ir.c1",
         "util.extract_ir.c3", "util.stale_copy"]
        + [f"util.pair_sum.n{n}" for n in (1, 255, 256, 4096 * 256 + 77)]
    ),
}
# seconds: each family takes a few seconds with its host reference; the limit only ends a run that hangs
LIMIT = {"a": 120, "b": 120, "r_int": 120, "r_f32": 120, "tap": 60, "c": 120, "util": 60}

_ended_badly = []   # (family, exit status) of a run that ended on a signal, its time limit or a HIP error (the program's status 3)


def _run(family):
    if _ended_badly:
        pytest.skip(f"family {_ended_badly[0][0]} ended with status {_ended_badly[0][1]}: nothing more is started on this GPU")
    assert os.path.isfile(EXE), "graphaudio_amd/conv_kernels_check is missing: the csrc Makefile's `all` target builds it"
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT[family]), EXE, family], capture_output=True, text=True)
    print(r.stdout[-20000:], r.stderr[-3000:])
    if r.returncode in (124, 137, 134, 139, 3) or r.returncode < 0:
        _ended_badly.append((family, r.returncode))
    checks, instances = {}, set()
    for line in r.stdout.splitlines():
        p = line.split()
        if len(p) >= 3 and p[0] == "check":
            checks[p[1]] = p[2]
        elif len(p) == 2 and p[0] == "instance":
            instances.add(p[1])
    failed = [k for k, v in checks.items() if v != "ok"]
    assert not failed, failed
    assert r.returncode == 0
    assert sorted(checks) == sorted(CHECKS[family])
    return instances


@pytest.mark.gpu
def test_a_is_exact_and_reads_only_what_the_planner_prepares():
    assert _run("a") == set()


@pytest.mark.gpu
def test_b_is_exact_on_integer_spectra():
    assert _run("b") == set()


@pytest.mark.gpu
def test_r_equals_float64_and_b_on_integer_spectra():
    assert _run("r_int") == set()


@pytest.mark.gpu
def test_r_is_the_reference_order_loop_bit_for_bit():
    assert _run("r_f32") == set()


@pytest.mark.gpu
def test_tap_spectra_every_instance_inside_the_transform_bound():
    assert sorted(_run("tap")) == sorted(TAP_INSTANCES)


@pytest.mark.gpu
def test_c_every_instance_inside_the_convolution_bound():
    assert sorted(_run("c")) == sorted(TAP_INSTANCES + C_INSTANCES)


@pytest.mark.gpu
def test_util_is_exact():
    assert _run("util") == set()
