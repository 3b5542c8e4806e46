"""The seven 256-point real-FFT kernel instances of the convolver path (graphaudio_amd/csrc/ga_rfft.hip) alone, against the float64
reference tests/rfft_ref.hpp.

tests/rfft_ref_kernels_main.hip drives them through their launchers on plain device tables, one family per process run, and prints
one line per check ("check <name> ok|FAIL <figures>").  Here every check must say ok and the set of check names must be the one
listed below (a case that was silently skipped fails).  The bounds are derived in the program's comments ("The
256-point transforms alone"): Higham's radix-2 bound for the transforms, the render tests' 2e-6 for the chain; the exact and seam
families compare bits.  tests/test_gpu_rfft_kernels.py stays the bit-level pin of the same kernels; this module is what says the
bits are right.  If a family ends on a signal or its time limit, the families behind it are skipped: nothing more is started on a
GPU that has just faulted."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "graphaudio_amd", "rfft_ref_check")

INSTANCES = ("a", "b32", "b64")
# (rows, blocks, hist of B, hist of A)
FWD_CASES = [(r, n, hb, ha) for r in (1, 31, 32, 33, 65) for n in (1, 3, 4, 5, 31, 32, 33, 64, 65) for hb, ha in ((0, 0), (4, 1), (512, 7))]
INV_CASES = [(r, n) for r in (1, 33, 65) for n in (1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 160, 161)]

CHECKS = {
    "fwd": [f"fwd.r{r}.n{n}.h{ha if i == 'a' else hb}.{i}" for r, n, hb, ha in FWD_CASES for i in INSTANCES],
    "inv": [f"inv.r{r}.n{n}.{i}" for r, n in INV_CASES for i in INSTANCES] + ["inv.migrate.b32", "inv.migrate.b64"],
    "exact": [f"exact.{s}.{i}" for s in ("fwd_columns", "inv_columns", "split.n97", "split.n161") for i in INSTANCES],
    "seam": ["seam.fwd_b32", "seam.fwd_b64", "seam.rebuild", "seam.inv_b32", "seam.inv_b64"],
    "chain": ["chain.b32", "chain.b64", "chain.a"],
}

_ended_badly = []   # (family, exit status) of a run that ended on a signal or its time limit


def _run(family):
    if _ended_badly:
        pytest.skip(f"family {_ended_badly[0][0]} ended with status {_ended_badly[0][1]}: nothing more is started on this GPU")
    assert os.path.isfile(EXE), "graphaudio_amd/rfft_ref_check is missing: the csrc Makefile's `all` target builds it"
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
def test_fwd_every_instance_against_the_float64_transform():
    _run("fwd")


@pytest.mark.gpu
def test_inv_every_instance_two_chunks_against_the_float64_transform():
    _run("inv")


@pytest.mark.gpu
def test_exact_equal_blocks_equal_columns_and_split_chunks():
    _run("exact")


@pytest.mark.gpu
def test_seam_every_row_behind_the_grid_limit_has_row_zeros_bits():
    _run("seam")


@pytest.mark.gpu
def test_chain_against_direct_convolution():
    _run("chain")
