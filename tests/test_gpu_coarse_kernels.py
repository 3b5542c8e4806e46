"""The kernels of formulation D (graphaudio_amd/csrc/ga_coarse.hip) alone, instance by instance, against the float64 reference
tests/coarse_ref.hpp.

tests/coarse_kernels_main.hip drives them through their launchers on plain device tables, one family per process run, and prints
one line per check ("check <name> ok|FAIL <figures>") and, for the multiply-accumulate family, one line per launch with the name
of the instance the launcher ran.  Here every check must say ok, the set of check names must be the one listed below (a case
that was silently skipped fails), and the set of instance names must be every instance launch_coarse_mac can dispatch to.  The
multiply-accumulate family is exact (integer spectra: float32 in any order equals float64); the other bounds are derived in the
program's comments ("The coarse kernels alone").  If a family ends on a signal or its time limit, the
families behind it are skipped: nothing more is started on a GPU that has just faulted."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "graphaudio_amd", "coarse_kernels_check")

INSTANCES = (
    [f"coarse_mac_kernel<{cw},{tw},{pb},8>" for cw in (1, 2) for tw, pb in [(2, 1)] + [(t, p) for t in (8, 9) for p in (1, 2, 4)]]
    + ["coarse_mac_kernel<4,2,1,8>", "coarse_mac_kernel<4,4,1,8>", "coarse_mac_kernel<4,4,2,8>", "coarse_mac_kernel<16,3,1,12>"]
    + [f"coarse_sum_kernel<{cw}>" for cw in (1, 2, 4)]
    + [f"coarse_mac_seg_kernel<{cw},{tw},4>" for cw in (1, 2) for tw in (2, 8, 9)]
    + ["coarse_mac_seg_kernel<4,2,4>", "coarse_mac_seg_kernel<4,4,4>"]
    + [f"coarse_sum_seg_kernel<{cw}>" for cw in (1, 2, 4)]
    + ["coarse_mfma16_kernel"]
)

CHECKS = {
    "mac": (
        [f"mac.c{cw}.tw2" for cw in (1, 2, 4)]
        + [f"mac.c{cw}.tw{tw}.pb{pb}" for cw in (1, 2) for tw in (8, 9) for pb in (1, 2, 4)]
        + ["mac.c4.tw4.pb1", "mac.c4.tw4.pb4"]
        + ["mac.c16.general", "mac.c16.general.bin0", "mac.c16.mfma.p1", "mac.c16.mfma.p1.bin0", "mac.c16.mfma.p4", "mac.c16.mfma.p4.bin0"]
        + [f"mac.sum.c{cw}" for cw in (1, 2, 4)]
        + [f"mac.seg.c{cw}.tw{tw}" for cw in (1, 2) for tw in (2, 8, 9)]
        + ["mac.seg.c4.tw2", "mac.seg.c4.tw4"]
        + [f"mac.sumseg.c{cw}" for cw in (1, 2, 4)]
    ),
    "mac_float": ["mac_float.mac", "mac_float.sum", "mac_float.seg", "mac_float.mfma16", "mac_float.mfma16.bin0"],
    "fwd": ["fwd.run_invariant", "fwd.unaligned_view", "fwd.carry", "fwd.handover", "fwd.constant", "fwd.alternating"]
    + [f"fwd.acc.{s}" for s in ("nohist", "hist1", "hist3", "nvalid128", "nvalid_cb_minus", "nvalid_cb_plus", "noin", "ir")],
    "inv": [f"inv.{s}" for s in ("ny1_nvalid128", "ny2_tail1", "ny3_tail3_out_only", "tail3_in_only", "short_ny", "no_tail", "zero_y")],
    "premix": [f"premix.{k}.w{w}" for k in ("int", "uni", "grid") for w in (1, 63, 64, 65, 4003)] + ["premix.handover"],
    "hist": [f"hist.{s}" for s in ("old_null", "in_null", "n_below", "n_equal", "n_above", "unaligned_in")],
    "chain": ["chain.convolution"],
}

_ended_badly = []   # (family, exit status) of a run that ended on a signal or its time limit


def _run(family):
    if _ended_badly:
        pytest.skip(f"family {_ended_badly[0][0]} ended with status {_ended_badly[0][1]}: nothing more is started on this GPU")
    assert os.path.isfile(EXE), "graphaudio_amd/coarse_kernels_check is missing: the csrc Makefile's `all` target builds it"
    r = subprocess.run(["timeout", "-k", "10", "120", EXE, family], capture_output=True, text=True)
    print(r.stdout[-12000:], r.stderr[-3000:])
    if r.returncode in (124, 137, 134, 139) or r.returncode < 0:
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
def test_mac_every_instance_is_exact_on_integer_spectra():
    instances = _run("mac")
    assert sorted(instances) == sorted(INSTANCES)
    assert len(set(INSTANCES)) == 33


@pytest.mark.gpu
def test_mac_float_stays_inside_the_inner_product_bound():
    _run("mac_float")


@pytest.mark.gpu
def test_fwd_identities_and_transform_bound():
    _run("fwd")


@pytest.mark.gpu
def test_inv_transform_bound_and_tail_routing():
    _run("inv")


@pytest.mark.gpu
def test_premix_is_exact_on_integers_and_inside_kahans_bound():
    _run("premix")


@pytest.mark.gpu
def test_hist_is_exact():
    _run("hist")


@pytest.mark.gpu
def test_chain_against_direct_convolution():
    _run("chain")
