"""The time-split biquad path of graphaudio_amd/csrc/ga_biquad.hip alone -- biquad_split_expand_kernel, the state-only and the full
lane kernels behind launch_biquad_lanes, biquad_scan_fixed_kernel<1..4> and biquad_scan_kernel -- against tests/biquad_split_ref.hpp,
bit for bit.

tests/biquad_split_main.hip drives the launchers on plain device tables, one family per process run, and prints one line per check
("check <name> ok|FAIL <figures>").  Here every check must say ok and the set of check names must be the one listed below (a case that
was silently skipped fails).
  scan    the scan kernels alone on integers, 1..8 sections, each length once through the fixed kernels (nsec = k) and once through the
          generic one (nsec = 0), G in {1, 2, 3, 5, 256}, 1..130 jobs: scratch and states exact, both launches the same bits
  expand  the passA / passB tables field by field, up to 258 threads, last piece full and short, twins
  pipe    expand -> pass A -> scan -> pass B in the planner's order, two segments in a row: outputs, scratch and persistent states equal
          to the scalar model on bits -- low cut-offs whose A^K is asserted to be >= 1 somewhere, so that a transposed matrix, a float
          accumulation or a z_l read one piece late cannot pass; mid-band cascades; an input that falls silent (subnormal states); more
          than 16,384 pieces in one launch; pipe.ragged.*: a last piece that is no multiple of 32 frames, which the planner never cuts
          and the kernels handle all the same
If a family ends on a signal, its time limit or a HIP error (exit status 3), the families behind it are skipped: nothing more is
started on a GPU that has just faulted.  ("The time-split biquad path alone".)"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "graphaudio_amd", "biquad_split_check")

SECTIONS = range(1, 9)
CHECKS = {
    "scan": [f"scan.s{k}.G{g}.n{n}" for k in SECTIONS for g in (1, 2, 3, 5, 256) for n in (1, 64, 65, 130)],
    "expand": [f"expand.c{c}xG{g}.{kl}.t{t}" for c, g in ((1, 2), (3, 3), (1, 256), (128, 2), (43, 6))
               for kl in ("K32.last32", "K1024.last1024", "K1024.last32") for t in (1, 2)],
    "pipe": (
        [f"pipe.s{k}.{c}" for k in SECTIONS
         for c in ("low.K32.G7.c65.t1", "low.K64.G3.c33.t2", "low.K96.G2.c1.t3", "low.K1056.G3.c33.t1", "mid.K1056.G7.c1.t2")]
        + ["pipe.s3.mid.K1056.G3.c1.t1.silent", "pipe.s2.low.K32.G256.c70.t1", "pipe.s8.low.K32.G256.c70.t1"]
        + [f"pipe.ragged.s{k}.r{r}" for k in (1, 3, 8) for r in (1, 3, 4, 31)]
    ),
}
# seconds: each family takes a few seconds with its host model; the limit only ends a run that hangs
LIMIT = {"scan": 120, "expand": 60, "pipe": 120}

_ended_badly = []   # (family, exit status) of a run that ended on a signal, its time limit or a HIP error (the program's status 3)


def _run(family):
    if _ended_badly:
        pytest.skip(f"family {_ended_badly[0][0]} ended with status {_ended_badly[0][1]}: nothing more is started on this GPU")
    assert os.path.isfile(EXE), "graphaudio_amd/biquad_split_check is missing: the csrc Makefile's `all` target builds it"
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT[family]), EXE, family], capture_output=True, text=True)
    print(r.stdout[-20000:], r.stderr[-3000:])
    if r.returncode in (124, 137, 134, 139, 3) or r.returncode < 0:
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


@pytest.mark.gpu
def test_expand_writes_the_piece_tables_and_nothing_else():
    _run("expand")


@pytest.mark.gpu
def test_scan_is_exact_on_integers_fixed_and_generic_alike():
    _run("scan")


@pytest.mark.gpu
def test_pipe_equals_the_scalar_model_bit_for_bit():
    _run("pipe")
