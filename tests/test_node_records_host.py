"""The node records (graphaudio_amd/csrc/ga_engine.hpp: NodeS and the per-type records derived from it), probed on the host: the
engine header compiles without the device compiler, and tests/node_records_main.cpp makes every node type's record through the
library's own factory (ga::makeNode) under a counting operator new and destroys it through the base pointer, as Context::nodes does.

What is pinned: a node is ONE allocation with the common part first; the only further allocations are the vectors the factory sizes
(inputs, outputs, params); only a stream source pays for stream queues; every record is smaller than the single record of all types it
replaced (1848 bytes, 5 allocations, 3000 bytes per node); the types without state of their own are the common record; and the typed
accessor refuses a node of another type with the engine's error instead of returning.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphaudio_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "node_records_main.cpp")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

PARENT_SIZEOF = 1848          # sizeof of the one record every node type shared before the split
GA_ERR_INVALID_ARGUMENT = -1
DESTINATION, BUFFER_SOURCE, GAIN, BIQUAD, CONVOLVER, SPLITTER, MERGER, CONSTANT, PANNER, OSCILLATOR, DELAY, STREAM, SPATIAL = range(13)
COMMON_ONLY = (DESTINATION, GAIN, SPLITTER, MERGER)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("node_records") / "node_records")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"),
                           "-I", CSRC, MAIN, "-x", "none", "-L", os.path.join(ROCM, "lib"), "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-lamdhip64",
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, check=True, text=True).stdout
    print(out)
    records, rest = {}, []
    for line in out.splitlines():
        w = line.split()
        if w[0] == "record":
            records[int(w[1])] = {w[i]: int(w[i + 1]) for i in range(2, len(w), 2)}
        else:
            rest.append(w)
    return records, rest


def test_every_type_has_a_record(probe):
    records, _ = probe
    assert sorted(records) == list(range(13))


def test_a_node_is_one_allocation_plus_the_vectors_the_factory_sizes(probe):
    records, _ = probe
    for t, r in records.items():
        assert r["first"] == r["sizeof"], t             # the record itself, whole: the common part and the typed part together
        if t != STREAM:
            assert r["allocs"] == 1 + r["vectors"], t   # inputs / outputs / params, where the type has any
        assert r["live"] == 0, t                        # destroyed through the base pointer: nothing is left behind


def test_only_a_stream_source_allocates_stream_queues(probe):
    records, _ = probe
    assert records[STREAM]["allocs"] > 1 + records[STREAM]["vectors"]     # its two deques (map and first page each)
    for t, r in records.items():
        if t != STREAM:
            assert r["allocs"] - 1 - r["vectors"] == 0, t


def test_every_record_is_smaller_than_the_record_of_all_types(probe):
    records, _ = probe
    for t, r in records.items():
        assert r["sizeof"] < PARENT_SIZEOF, t


def test_types_without_state_are_the_common_record(probe):
    records, rest = probe
    common = [int(w[1]) for w in rest if w[0] == "common"]
    assert len(common) == 1
    for t, r in records.items():
        if t in COMMON_ONLY:
            assert r["sizeof"] == common[0], t
        else:
            assert r["sizeof"] > common[0], t


def test_accessor_refuses_the_wrong_type(probe):
    _, rest = probe
    assert not [w for w in rest if w[0] == "returned"]
    mism = [w for w in rest if w[0] == "mismatch"]
    assert len(mism) == 2                               # rec<DelayS>(gain) and schedOf(gain)
    for w in mism:
        assert int(w[1]) == GA_ERR_INVALID_ARGUMENT and "wrong type" in " ".join(w[2:])
    assert [w for w in rest if w[0] == "matched"]       # ... and hands out the record of the right one
