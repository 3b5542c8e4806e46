"""The decisions of the graph analysis (graphaudio_amd/csrc/ga_topology.cpp; Context::chunkTopology drives it) against a record taken
on the commit before the analysis became a module of its own: tools/record_topology_decisions.py renders thirteen scenes -- loops cut
at delays and loops that cannot be cut, modulated rates with loops outside and inside their cone, `delay_flag_exact` 1 and 2, a
SpatialPannerNode with signals on its parameters, a generated graph with feedback -- each in one call and in three uneven pieces.
tests/golden/topology_decisions.json holds what that commit decided (chunks, segments, launches, flags read and predicted) and the
SHA-256 of what it rendered; recorded twice there, every hash reproduced.  All of it has to be equal: the kernels on these paths sum
in a fixed order."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_topology_decisions", os.path.join(ROOT, "tools", "record_topology_decisions.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()
with open(os.path.join(ROOT, "tests", "golden", "topology_decisions.json"), encoding="utf-8") as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def record():
    return REC.record()


def test_every_scene_is_recorded(record):
    assert sorted(record) == sorted(GOLDEN) and len(GOLDEN) == 26


@pytest.mark.parametrize("key", sorted(GOLDEN))
def test_decisions_and_samples_are_those_of_the_parent_commit(record, key):
    got, want = record[key], GOLDEN[key]
    print(key, got)
    assert want["rms"] > 1e-3   # (the scene is heard)
    for counter in REC.COUNTERS:
        assert got[counter] == want[counter], (counter, got[counter], want[counter])
    assert got["sha256"] == want["sha256"]
