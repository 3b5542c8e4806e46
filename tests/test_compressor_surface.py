"""DynamicsCompressorNode: the public surface -- Python host, C header, C# binding.  No GPU needed."""
import os
import re

import numpy as np
import pytest

from tests import _compressor_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the definition's table: (name, default, min, max), all k-rate
DEFINITION = [("threshold", -24.0, -100.0, 0.0), ("knee", 30.0, 0.0, 40.0), ("ratio", 12.0, 1.0, 20.0),
              ("attack", 0.003, 0.0, 1.0), ("release", 0.25, 0.0, 1.0), ("makeupGain", 0.0, -40.0, 40.0)]
HEADER_NAMES = ["THRESHOLD", "KNEE", "RATIO", "ATTACK", "RELEASE", "MAKEUP_GAIN"]


def _header():
    return open(os.path.join(ROOT, "include", "graphaudio_hip.h")).read()


def test_python_class_has_the_definitions_parameters_and_defaults():
    from graphaudio_amd import AudioNode, DynamicsCompressorNode
    assert issubclass(DynamicsCompressorNode, AudioNode)
    assert [tuple(p) for p in DynamicsCompressorNode.PARAMS] == DEFINITION
    assert [tuple(p) for p in M.PARAMS] == DEFINITION   # (the model the GPU tests compare with clamps to the same ranges)


def test_python_parameters_are_krate_audio_params_in_native_order():
    """on the CPU oracle's API a node type the oracle does not know cannot be created: the normal exception.  The compressor it
    knows (tests/test_oracle_compressor.py): six k-rate parameters in the native order with the header's defaults"""
    from graphaudio_amd import ArgumentException, DynamicsCompressorNode, SpatialPannerNode
    from tests._oracle import OracleContext
    ctx = OracleContext(48000)
    with pytest.raises(ArgumentException):
        SpatialPannerNode(ctx)
    on_oracle = DynamicsCompressorNode(ctx)
    hdr = _header()
    for i, (name, default, mn, mx) in enumerate(DEFINITION):
        p = [on_oracle.Threshold, on_oracle.Knee, on_oracle.Ratio, on_oracle.Attack, on_oracle.Release, on_oracle.MakeupGain][i]
        assert p._index == i and p.Name == name
        assert p.Value == np.float32(default)   # (read back through gao_param_get_value: the oracle's own default)
        m = re.search(r"GA_COMPRESSOR_%s\s+default\s+(-?[\d.]+)" % HEADER_NAMES[i], hdr)
        assert m and float(m.group(1)) == default, name
        for v, want in ((mn - 1.0, mn), (mx + 1.0, mx)):   # ... and the oracle's own range
            p.Value = v
            assert p.Value == want
    with pytest.raises(ArgumentException):
        ctx._call("param_set_value", on_oracle.NodeId, 6, 0.0)   # (there is no seventh)

    # the parameter objects, on a context stand-in that records the calls instead of making them
    class Recorder:
        SampleRate = 48000

        def __init__(self):
            self._nodes, self.calls = {}, []

        def _call(self, fn, *args):
            self.calls.append((fn, args))
            if fn == "node_create":
                args[1]._obj.value = 7
            return 0
    from graphaudio_amd import AudioParam, AutomationRate, _capi
    rec = Recorder()
    cm = DynamicsCompressorNode(rec)
    assert rec.calls[0][0] == "node_create" and rec.calls[0][1][0] == _capi.NODE_DYNAMICS_COMPRESSOR and cm.NodeId == 7
    props = [cm.Threshold, cm.Knee, cm.Ratio, cm.Attack, cm.Release, cm.MakeupGain]
    for i, (p, (name, default, mn, mx)) in enumerate(zip(props, DEFINITION)):
        assert isinstance(p, AudioParam) and p._index == i
        assert (p.Name, p.DefaultValue, p.MinValue, p.MaxValue, p.AutomationRate) == (name, default, mn, mx, AutomationRate.KRate)
    cm.Ratio.Value = 4.0
    assert rec.calls[-1] == ("param_set_value", (7, _capi.COMPRESSOR_RATIO, 4.0))


def test_capi_constants_equal_the_headers():
    from graphaudio_amd import DynamicsCompressorNode, _capi
    hdr = _header()
    m = re.search(r"GA_NODE_DYNAMICS_COMPRESSOR\s*=\s*(\d+)", hdr)
    assert m and int(m.group(1)) == 13 == _capi.NODE_DYNAMICS_COMPRESSOR == DynamicsCompressorNode._node_type
    for i, name in enumerate(HEADER_NAMES):
        m = re.search(r"GA_COMPRESSOR_%s\s*=\s*(\d+)" % name, hdr)
        assert m and int(m.group(1)) == i == getattr(_capi, "COMPRESSOR_" + name), name
    m = re.search(r"GA_COMPRESSOR_PARAM_COUNT\s*=\s*(\d+)", hdr)
    assert m and int(m.group(1)) == 6 == _capi.COMPRESSOR_PARAM_COUNT
    # every node type value of the header is used once
    values = [int(v) for v in re.findall(r"GA_NODE_\w+\s*=\s*(\d+)", hdr)]
    assert sorted(values) == list(range(14))
    # the definition is in the header's comment block
    for word in ("GA_COMPRESSOR_THRESHOLD", "log10", "look-ahead", "GA_ERR_UNSUPPORTED"):
        assert word in hdr[hdr.index("DynamicsCompressorNode"):hdr.index("GA_NODE_DYNAMICS_COMPRESSOR = 13")]


def test_header_declares_no_new_entry_point():
    names = re.findall(r"GA_EXPORT[^;]*?GA_FN\((\w+)\)", _header(), flags=re.S)
    assert not [n for n in names if "compress" in n.lower() or "dynamics" in n.lower()]


def test_csharp_binding_carries_the_same_values():
    cs = open(os.path.join(ROOT, "bindings", "csharp", "GraphAudioHip.cs")).read()
    m = re.search(r"NodeDynamicsCompressor\s*=\s*(\d+)", cs)
    assert m and int(m.group(1)) == 13
    for i, name in enumerate(["Threshold", "Knee", "Ratio", "Attack", "Release", "MakeupGain"]):
        m = re.search(r"Compressor%s\s*=\s*(\d+)" % name, cs)
        assert m and int(m.group(1)) == i, name
    wrapper = open(os.path.join(ROOT, "bindings", "csharp", "HipOfflineAudioContext.cs")).read()
    assert "class DynamicsCompressorNode" in wrapper and "GraphAudioHip.NodeDynamicsCompressor" in wrapper
    body = wrapper[wrapper.index("class DynamicsCompressorNode"):]
    for name, default, mn, mx in DEFINITION:
        assert re.search(r'\("%s",\s*%sf,\s*%sf,\s*%sf\)' % (name, *(re.escape(("%g" % v)) for v in (default, mn, mx))), body), name
