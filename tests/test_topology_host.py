"""The graph analysis of a chunk (graphaudio_amd/csrc/ga_topology.cpp) on the host alone: tests/topology_main.cpp builds small graphs
from the library's node records and checks order, levels, convolver depths, stale producers, the loop gain bound, the chunk length of
loops cut at their DelayNodes, the delays `delay_flag_exact` accepts and keeps, and the rate cones and their roots.  The module and
the program are compiled by the host compiler under the address and undefined-behaviour sanitizers; nothing is loaded into Python."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphaudio_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_graph_analysis_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "topology")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "topology_main.cpp"), os.path.join(CSRC, "ga_topology.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok"


def test_the_module_calls_no_device_function_and_no_context_member():
    with open(os.path.join(CSRC, "ga_topology.cpp"), encoding="utf-8") as f:
        code = "\n".join(line.split("//")[0] for line in f.read().splitlines())
    assert not re.search(r"\bhip[A-Z]\w*\s*\(|\bGA_HIP\b|\bContext\b", code)
