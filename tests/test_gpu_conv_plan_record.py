"""The fine-partition side of the convolver planner (graphaudio_amd/csrc/ga_plan_conv.cpp: the shared-IR groups of formulation A, the
private-IR stage of formulations B / C / R, the conv_migrate rebuild) against a record taken on the commit before the private-IR stage
was split into passes: the "conv" table of tools/record_topology_decisions.py renders eight scenes -- eight voices on a shared
response with one input materialised; private responses of 1, 2 and 17 partitions behind mono, stereo, true-stereo and late-starting
inputs; 17 columns on one x-row; 65 partitions on formulation C with the mixed radix-16 plan and with radix 2; the true-stereo scene
of test_gpu_reforder.py on formulation R; a mono input whose channels start to differ between two calls; a migrating convolver --
each in one call and in three uneven pieces, every scene over at least three chunks.  tests/golden/conv_plan_decisions.json holds
what that commit planned (chunks, segments, launches, partition-sum launches, flops and bytes, reference-order rows, migrations,
shared rows) and the SHA-256 of what it rendered; recorded twice there, every hash reproduced.  All of it has to be equal: these
kernels sum in a fixed order."""
import json
import os

import pytest

from tests.test_gpu_topology_record import REC, ROOT

pytestmark = pytest.mark.gpu

with open(os.path.join(ROOT, "tests", "golden", "conv_plan_decisions.json"), encoding="utf-8") as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def record():
    return REC.record(table=REC.conv_scenes, counters=REC.CONV_COUNTERS)


def test_every_scene_is_recorded(record):
    assert sorted(record) == sorted(GOLDEN) and len(GOLDEN) == 16
    for family in ("a_", "b_", "c_", "r_", "hand_down_", "migrate_"):
        assert any(k.startswith(family) for k in GOLDEN), family


@pytest.mark.parametrize("key", sorted(GOLDEN))
def test_plan_and_samples_are_those_of_the_parent_commit(record, key):
    got, want = record[key], GOLDEN[key]
    print(key, got)
    assert want["rms"] > 1e-3   # (the scene is heard)
    for counter in REC.CONV_COUNTERS:
        assert got[counter] == want[counter], (counter, got[counter], want[counter])
    assert got["sha256"] == want["sha256"]
