"""The four SpatialPannerNode kernels (graphaudio_amd/csrc/ga_spatial.hip) alone, against tests/spatial_ref.hpp.

The node has no counterpart in the reference: no oracle renders it and the fuzzer does not draw it.  The render tests hold it to a
Python model within 1e-5 of the peak; tests/spatial_kernels_main.hip drives the launchers on plain device tables, one family per
process run, and prints one line per check ("check <name> ok|FAIL <figures>").  Here every check must say ok and the set of check
names must be the one listed below (a case that was silently skipped fails).  panner compares every written sample with the float64
statement of the contract on inputs on which float32 is exact; float compares bits with the float32 chain ga_kernels.hpp promises
and holds them to a derived bound of the float64 form; direct compares bits with the host walk of ga_spatial_direct.hpp; desc and
head compare with ga_spatial_geom.hpp / ga_spatial_head.hpp on the host.  The cases and bounds are in the program's comments and in
DESIGN.md section 4, "The SpatialPannerNode kernels alone".  If a family ends on a signal or its time limit, the families behind it
are skipped: nothing more is started on a GPU that has just faulted."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "graphaudio_amd", "spatial_kernels_check")

CHECKS = {
    "panner": [f"panner.T{t}.n{n}" for t in (1, 2, 3, 127, 128, 129, 511, 512) for n in (1, 3, 4, 5, 9)]
    + [f"panner.silent.{w}.T{t}" for t in (3, 129, 512) for w in ("plan", "span")]
    + [f"panner.hist.T512.n{n}" for n in (1, 2, 3)] + ["panner.cut.T129", "panner.cut.T512"],
    "float": [f"float.T{t}.{c}.{f}" for t in (129, 512) for c in ("mono", "stereo") for f in ("steady", "fade")],
    "direct": ["direct.n1", "direct.n8", "direct.n9", "direct.identity.mono", "direct.identity.stereo", "direct.active0", "direct.restart",
               "direct.carry_job", "direct.carry_job_half", "direct.carry_state", "direct.prev_invalid", "direct.cut"],
    "desc": [f"desc.value.nb{n}" for n in (1, 63, 64, 65)] + ["desc.curve.nb65", "desc.mod", "desc.two_jobs", "desc.cone", "desc.cone_exponential",
                                                                "desc.eq", "desc.prev.none", "desc.prev.host", "desc.prev.in_b0", "desc.prev.in_b2",
                                                                "desc.prev.chain"],
    "head": [f"head.t{t}.s{s}" for t in (1, 63, 64, 65, 512) for s in (0, 3)],
}

_ended_badly = []   # (family, exit status) of a run that ended on a signal or its time limit


def _run(family):
    if _ended_badly:
        pytest.skip(f"family {_ended_badly[0][0]} ended with status {_ended_badly[0][1]}: nothing more is started on this GPU")
    assert os.path.isfile(EXE), "graphaudio_amd/spatial_kernels_check is missing: the csrc Makefile's `all` target builds it"
    r = subprocess.run(["timeout", "-k", "10", "120", EXE, family], capture_output=True, text=True)
    print(r.stdout[-30000:], r.stderr[-3000:])
    if r.returncode in (124, 137, 134, 139) or r.returncode < 0:
        _ended_badly.append((family, r.returncode))
    checks = {}
    for line in r.stdout.splitlines():
        p = line.split()
        if len(p) >= 3 and p[0] == "check":
            checks[p[1]] = p[2]
    failed = [k for k, v in checks.items() if v != "ok"]
    assert not failed, failed
    assert r.returncode == 0
    assert sorted(checks) == sorted(CHECKS[family])
    assert len(set(CHECKS[family])) == len(CHECKS[family])


@pytest.mark.gpu
def test_panner_every_written_sample_is_the_float64_value():
    _run("panner")


@pytest.mark.gpu
def test_float_bits_of_the_fma_chain_within_the_derived_bound():
    _run("float")


@pytest.mark.gpu
def test_direct_bit_for_bit_against_the_host_walk():
    _run("direct")


@pytest.mark.gpu
def test_desc_against_the_geometry_on_the_host():
    _run("desc")


@pytest.mark.gpu
def test_head_every_tap_against_the_host():
    _run("head")
